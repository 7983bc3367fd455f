"""What the derivatives of the rigid-body plant cost: Plan.srb_vjp with every output and with
g_x alone and Plan.srb_jvp with every tangent, at nsub = 20, on 65,536 robots (config 3's size) and
on 1,024, next to Plan.srb_step itself, a device-to-device copy of the bytes each entry reads and
writes, and a cold solve step of config 3 at the same batch, all in one process.

The robots are in general position (tilted, moving, turning, their own mass, inertia and gait);
the forces are read off the rows of the solve's w with row stride 24 N, as the closed loop reads
them.  The gradients and tangents are fixed random arrays.  Each round times the variants one after
the other with HIP events (--reps launches per event pair), after --warmup untimed rounds; the
record holds the median and the min / max over --rounds rounds, the bytes per robot and each ratio
to its copy and to the cold solve.  A copy of n bytes reads n and writes n, so it moves twice the
bytes of the entry it stands next to (the convention of dynamics_grad_bench.py).  Plan.srb_step
advances its state in place, so its robots move on from call to call; its time does not depend on
where they are.  There is no time bar: these are new entries.
   usage: python tools/srb_grad_bench.py [--batches 65536,1024] [--nsub 20] [--rounds 10]
                                   [--warmup 3] [--reps 5] [--out profiles/srb_grad_bench.json]"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "convex-mpc-unitree-go2_amd"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cmpc import Plan, SolverParams, synth, to_device_batch  # noqa: E402

from bench_util import emit, interleaved_rounds, solve_steps  # noqa: E402

# bytes per robot: t_now, gait fp64; mass, inertia, force, x, feet fp32; contact_state
INPUTS = 8 * (1 + 6) + 4 * (1 + 9 + 12 + 12 + 12) + 1
TRAFFIC = {"vjp": (INPUTS + 8 * 24, 8 * (12 + 12 + 12 + 1 + 9)),
           "vjp_x": (INPUTS + 8 * 24, 8 * 12),
           "jvp": (INPUTS + 4 * (12 + 12 + 12 + 1 + 9), 4 * 24),
           "primal": (INPUTS, 4 * 24 + 1)}


def plant_inputs(B, seed, dev):
    """B robots in general position on the device (the distribution of the plant's tests)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 12))
    x[:, 0:2] = rng.uniform(-1, 1, (B, 2))
    x[:, 2] = synth.Z_DES + rng.uniform(-0.02, 0.02, B)
    x[:, 3:5] = rng.uniform(-0.3, 0.3, (B, 2))
    x[:, 5] = rng.uniform(-np.pi, np.pi, B)
    x[:, 6:9] = rng.uniform(-0.7, 0.7, (B, 3))
    x[:, 9:12] = rng.uniform(-2, 2, (B, 3))
    S = rng.normal(0, 0.03, (B, 3, 3))
    Ib = synth.INERTIA_BODY[None] + (S + np.swapaxes(S, 1, 2)) / 2
    hip = np.asarray(synth.HIP_OFFSETS)
    c, s = np.cos(x[:, 5]), np.sin(x[:, 5])
    feet = np.stack([np.stack([x[:, 0] + c * hx - s * hy, x[:, 1] + s * hx + c * hy,
                               np.zeros(B)], -1) for hx, hy in hip[:, :2]], 1)
    gait = np.concatenate([rng.uniform(0.25, 0.5, (B, 1)), rng.uniform(0.4, 0.8, (B, 1)),
                           rng.uniform(0, 1, (B, 4))], 1)
    f32, f64 = torch.float32, torch.float64
    put = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)  # noqa: E731
    return dict(t_now=put(rng.uniform(0, 1000, B), f64), gait=put(gait, f64),
                mass=put(rng.uniform(10, 20, B), f32), inertia_body=put(Ib, f32), hip=put(hip, f32),
                x=put(x, f32), feet=put(feet, f32),
                contact_state=put(rng.integers(0, 16, B), torch.uint8))


def measure(plan, B, nsub, a):
    dev, N = plan.device, plan.params.N
    d = to_device_batch(synth.make_config(3, B=B), dev)
    solve = solve_steps(plan, d, a.rounds, a.warmup)
    w, _, _ = plan.solve(d["Ad"], d["Bd"], d["gd"], d["x0"], d["xref"], d["contact"])
    p = plant_inputs(B, 11, dev)
    h = (1.0 / 3 / N) / nsub
    ins = lambda x, feet, cs: (p["t_now"], p["gait"], p["mass"], p["inertia_body"], w[:, 12 * N:],  # noqa: E731
                               p["hip"], x, feet, cs, nsub, h)
    pre = ins(p["x"], p["feet"], p["contact_state"])
    gen = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda shape, dtype: torch.randn(shape, dtype=dtype, device=dev, generator=gen)  # noqa: E731
    f32, f64 = torch.float32, torch.float64
    grads = dict(g_x=rnd((B, 12), f64), g_feet=rnd((B, 4, 3), f64))
    tan = dict(x=rnd((B, 12), f32), feet=rnd((B, 4, 3), f32), force=rnd((B, 12), f32),
               mass=rnd((B,), f32), inertia_body=rnd((B, 3, 3), f32))
    vres = plan.srb_vjp(*pre, **grads)
    xres = plan.srb_vjp(*pre, **grads, want=("x",))
    jres = plan.srb_jvp(*pre, tan)
    moving = ins(p["x"].clone(), p["feet"].clone(), p["contact_state"].clone())
    nbytes = {k: sum(v) for k, v in TRAFFIC.items()}
    src = {k: torch.empty(B * n, dtype=torch.uint8, device=dev).random_(0, 256)
           for k, n in nbytes.items()}
    dst = {k: torch.empty_like(v) for k, v in src.items()}
    variants = {"vjp": (lambda: plan.srb_vjp(*pre, **grads, out=vres), a.reps),
                "vjp_x": (lambda: plan.srb_vjp(*pre, **grads, want=("x",), out=xres), a.reps),
                "jvp": (lambda: plan.srb_jvp(*pre, tan, out=jres), a.reps),
                "primal": (lambda: plan.srb_step(*moving), a.reps)}
    for k in nbytes:
        variants["copy_" + k] = (lambda k=k: dst[k].copy_(src[k]), a.reps)
    rec = {"batch": B, "nsub": nsub, "cold_solve": solve}
    rec.update(interleaved_rounds(variants, a.warmup, a.rounds))
    for k, (rd, wr) in TRAFFIC.items():
        rec[k]["bytes_read_per_robot"], rec[k]["bytes_written_per_robot"] = rd, wr
        rec[k]["bytes_moved_GBps"] = (rd + wr) * B / (rec[k]["ms"] * 1e6)
        rec[k]["ratio_to_copy"] = rec[k]["ms"] / rec["copy_" + k]["ms"]
        rec[k]["ratio_to_cold_solve"] = rec[k]["ms"] / solve["ms_per_step"]
        rec["copy_" + k]["bytes"] = 2 * nbytes[k] * B       # a copy reads and writes each byte
    torch.cuda.synchronize(dev)
    rec["nan_robots"] = int(sum(torch.isnan(v.reshape(B, -1)).any(1).sum() for v in vres.values()))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=str, default="65536,1024")
    ap.add_argument("--nsub", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=str(REPO / "profiles" / "srb_grad_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("srb_grad_bench: no ROCm device (nothing is measured without one)")
    batches = [int(b) for b in a.batches.split(",")]
    plan = Plan(SolverParams(max_batch=max(batches)))
    rec = {"config": 3, "N": plan.params.N, "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(plan.device),
           "runs": [measure(plan, B, a.nsub, a) for B in batches]}
    emit(rec, a.out)


if __name__ == "__main__":
    main()
