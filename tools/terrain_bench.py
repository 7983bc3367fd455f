"""What heterogeneous terrain costs: config 3 (65,536 QPs) solved cold with per-instance
mu / fz_min from synth.make_terrain against the same batch with the plan's constants (NULL
arrays).  Prints and optionally writes one JSON record: ms per step, the status histogram and
the mean / max ADMM iterations of each.
   usage: python tools/terrain_bench.py [--batch 65536] [--steps 10] [--warmup 3] [--out FILE]"""
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
    a = ap.parse_args()
    plan = Plan(SolverParams(max_batch=a.batch))
    batch = synth.make_config(3, B=a.batch)
    batch.update(synth.make_terrain(a.batch, a.seed))
    d = to_device_batch(batch, plan.device)
    rec = {"config": 3, "batch": a.batch, "steps": a.steps, "warmup": a.warmup,
           "terrain": {"seed": a.seed, "mu": [0.2, 1.0], "fz_min": [0.0, 20.0]},
           "device": torch.cuda.get_device_name(plan.device),
           "plan_constants": solve_steps(plan, d, a.steps, a.warmup),
           "per_instance": solve_steps(plan, d, a.steps, a.warmup, mu=d["mu"], fz_min=d["fz_min"])}
    rec["ratio"] = rec["per_instance"]["ms_per_step"] / rec["plan_constants"]["ms_per_step"]
    emit(rec, a.out)


if __name__ == "__main__":
    main()
