"""What the derivatives of the dynamics builder cost: Plan.dynamics_vjp with every output and
Plan.dynamics_jvp with every tangent on config 3 (65,536 robots), next to Plan.build_dynamics and
a device-to-device copy of the bytes each of the three reads and writes, all in one process.

The gradients are fixed random fp64 arrays, the tangents fixed random fp32 arrays.  Each round
times the variants one after the other with HIP events (--reps launches per event pair), after
--warmup untimed rounds; the record holds the median and the min / max over --rounds rounds, the
bytes per robot and each ratio to its copy.  A copy of n bytes reads n and writes n, so it moves
twice the bytes of the entry it stands next to (the convention of jvp_bench.py); bytes_moved_GBps
is the entry's own bytes over its own time.  There is no time bar.
   usage: python tools/dynamics_grad_bench.py [--batch 65536] [--rounds 10] [--warmup 3]
                                    [--reps 5] [--out profiles/dynamics_grad_bench.json]"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "convex-mpc-unitree-go2_amd"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cmpc import Plan, SolverParams, synth  # noqa: E402

from bench_util import emit, interleaved_rounds  # noqa: E402


def traffic(N):
    """name -> (bytes read, bytes written) per robot: the inputs of cmpc_build_dynamics (fp32; of
    xref the yaw column's 32-byte sectors are what a row costs, counted whole here), then each
    entry's own arrays."""
    inputs = 4 * (1 + 9 + 12 * N + 12 * N)
    return {"vjp": (inputs + 8 * (144 + 144 * N), 8 * (1 + 9 + 12 * N + 1)),
            "jvp": (2 * inputs, 4 * (144 + 144 * N)),
            "primal": (inputs, 4 * (144 + 144 * N + 12))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=str(REPO / "profiles" / "dynamics_grad_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dynamics_grad_bench: no ROCm device (nothing is measured without one)")
    B = a.batch
    plan = Plan(SolverParams(max_batch=8))                # (max_batch does not limit these entries)
    N = plan.params.N
    dev = plan.device
    b = synth.make_config(3, B=B)
    args = [torch.as_tensor(np.ascontiguousarray(b[k]), dtype=torch.float32).to(dev)
            for k in ("m", "I_world", "r_legs", "xref")] + [float(b["dt"])]
    gen = torch.Generator(device=dev).manual_seed(5)
    g_Ad = torch.randn((B, 12, 12), dtype=torch.float64, device=dev, generator=gen)
    g_Bd = torch.randn((B, N, 12, 12), dtype=torch.float64, device=dev, generator=gen)
    tan = {n: torch.randn(t.shape, dtype=torch.float32, device=dev, generator=gen)
           for n, t in zip(("mass", "inertia", "r_feet", "xref"), args[:4])}
    vres = plan.dynamics_vjp(*args, g_Ad=g_Ad, g_Bd=g_Bd)
    jres = plan.dynamics_jvp(*args, tan)
    pres = plan.build_dynamics(*args)
    nbytes = {k: sum(v) for k, v in traffic(N).items()}
    src = {k: torch.empty(B * n, dtype=torch.uint8, device=dev).random_(0, 256)
           for k, n in nbytes.items()}
    dst = {k: torch.empty_like(v) for k, v in src.items()}
    variants = {"vjp": (lambda: plan.dynamics_vjp(*args, g_Ad=g_Ad, g_Bd=g_Bd, out=vres), a.reps),
                "jvp": (lambda: plan.dynamics_jvp(*args, tan, out=jres), a.reps),
                "primal": (lambda: plan.build_dynamics(*args, out=pres), a.reps)}
    for k in nbytes:
        variants["copy_" + k] = (lambda k=k: dst[k].copy_(src[k]), a.reps)
    rec = {"config": 3, "batch": B, "N": N, "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(dev)}
    rec.update(interleaved_rounds(variants, a.warmup, a.rounds))
    for k, (rd, wr) in traffic(N).items():
        rec[k]["bytes_read_per_robot"], rec[k]["bytes_written_per_robot"] = rd, wr
        rec[k]["bytes_moved_GBps"] = (rd + wr) * B / (rec[k]["ms"] * 1e6)
        rec[k]["ratio_to_copy"] = rec[k]["ms"] / rec["copy_" + k]["ms"]
        rec["copy_" + k]["bytes"] = 2 * nbytes[k] * B       # a copy reads and writes each byte
        rec["copy_" + k]["bytes_moved_GBps"] = 2 * nbytes[k] * B / (rec["copy_" + k]["ms"] * 1e6)
    torch.cuda.synchronize(dev)
    rec["nan_robots"] = int(sum(torch.isnan(t.reshape(B, -1)).any(1).sum() for t in vres.values()))
    emit(rec, a.out)


if __name__ == "__main__":
    main()
