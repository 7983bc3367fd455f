"""What per-robot cost weights cost: config 3 (65,536 QPs) solved cold with per-instance Q / R
from synth.make_weights against the same batch with the plan's constants (NULL arrays), and the
same batch with arrays filled with the plan's constants (the price of the per-instance read
alone).  Prints and optionally writes one JSON record: ms per step, the status histogram and the
mean / max ADMM iterations of each.  --null-only measures the NULL path alone, --repeat times
over (the run-to-run spread of the headline path, for an A/B against another build).
   usage: python tools/weights_bench.py [--batch 65536] [--steps 10] [--warmup 3] [--out FILE]
                                        [--null-only] [--repeat 1]"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "convex-mpc-unitree-go2_amd"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

from cmpc import Plan, SolverParams, synth, to_device_batch  # noqa: E402

from bench_util import emit, solve_steps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--null-only", action="store_true")
    ap.add_argument("--repeat", type=int, default=1)
    a = ap.parse_args()
    plan = Plan(SolverParams(max_batch=a.batch))
    batch = synth.make_config(3, B=a.batch)
    d = to_device_batch(batch, plan.device)
    rec = {"config": 3, "batch": a.batch, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(plan.device),
           "plan_constants": [solve_steps(plan, d, a.steps, a.warmup) for _ in range(a.repeat)]}
    if not a.null_only:
        wt = synth.make_weights(a.batch, a.seed)
        f32 = torch.float32
        Q, R = (torch.as_tensor(wt[k], dtype=f32).contiguous().to(plan.device) for k in ("Q", "R"))
        p = plan.params
        Qc, Rc = (torch.tensor(v, dtype=f32).expand(a.batch, 12).contiguous().to(plan.device)
                  for v in (p.Q, p.R))
        rec["weights"] = {"seed": a.seed, "q_span": 4.0, "r": [2.5e-6, 1e-4]}
        rec["constant_arrays"] = solve_steps(plan, d, a.steps, a.warmup, Q=Qc, R=Rc)
        rec["per_instance"] = solve_steps(plan, d, a.steps, a.warmup, Q=Q, R=R)
        rec["ratio"] = rec["per_instance"]["ms_per_step"] / rec["plan_constants"][0]["ms_per_step"]
    emit(rec, a.out)


if __name__ == "__main__":
    main()
