"""What the derivatives of the trajectory generator cost: Plan.traj_vjp with every gradient and
output and Plan.traj_jvp with every tangent and output on config 3's tick inputs (65,536 robots:
even robots the shared trot, odd robots mixed gaits), next to Plan.generate_traj and a
device-to-device copy of the bytes each of the three reads and writes, all in one process.

The gradients are fixed random fp64 arrays, the tangents fixed random arrays of their dtypes.
Each round times the variants one after the other with HIP events (--reps launches per event
pair), after --warmup untimed rounds; the record holds the median and the min / max over --rounds
rounds, the bytes per robot and each ratio to its copy.  A copy of n bytes reads n and writes n,
so it moves twice the bytes of the entry it stands next to (the convention of
dynamics_grad_bench.py); bytes_moved_GBps is the entry's own bytes over its own time.  There is no
time bar.
   usage: python tools/traj_grad_bench.py [--batch 65536] [--rounds 10] [--warmup 3]
                                    [--reps 5] [--out profiles/traj_grad_bench.json]"""
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

F64 = ("pos_des", "t_now", "gait")


def traffic(N):
    """name -> (bytes read, bytes written) per robot: the per-robot inputs of cmpc_generate_traj
    (x0 and cmd fp32, pos_des, t_now and gait fp64; hip is 48 bytes for the whole batch), then
    each entry's own arrays."""
    inputs = 4 * (12 + 4) + 8 * (3 + 1 + 6)
    return {"vjp": (inputs + 8 * (12 * N + 12 * N + 1 + 3), 8 * (12 + 3 + 4 + 12)),
            "jvp": (inputs + 4 * (12 + 4 + 12) + 8 * 3, 4 * (12 * N + 12 * N) + 8 * 3),
            "primal": (inputs + 4 * 12, 4 * (12 * N + 12 * N) + 4 * N + 8 * 3)}


def tick_inputs(B, N):
    """Config 3's mix as tick inputs: even robots make_tick_inputs(mixed=False), odd robots
    mixed=True, with config 3's seeds + 500."""
    a = synth.make_tick_inputs((B + 1) // 2, seed=3 + 500, mixed=False, N=N)
    b = synth.make_tick_inputs(B // 2, seed=1003 + 500, mixed=True, N=N)
    out = {"hip": a["hip"], "dt": a["dt"]}
    for k in ("x0", "pos_des", "cmd", "t_now", "gait", "foot_lever"):
        out[k] = np.empty((B,) + a[k].shape[1:])
        out[k][0::2], out[k][1::2] = a[k], b[k]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=str(REPO / "profiles" / "traj_grad_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("traj_grad_bench: no ROCm device (nothing is measured without one)")
    B = a.batch
    plan = Plan(SolverParams(max_batch=8))                # (max_batch does not limit these entries)
    N = plan.params.N
    dev = plan.device
    t = tick_inputs(B, N)
    td = {k: torch.as_tensor(np.ascontiguousarray(t[k]),
                             dtype=torch.float64 if k in F64 else torch.float32).to(dev)
          for k in ("x0", "pos_des", "cmd", "t_now", "gait", "foot_lever", "hip")}
    dt = float(t["dt"])
    ins = [td[k] for k in ("x0", "pos_des", "cmd", "t_now", "gait", "hip")]
    gen = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda shape, dtype: torch.randn(shape, dtype=dtype, device=dev, generator=gen)  # noqa: E731
    f32, f64 = torch.float32, torch.float64
    grads = dict(g_xref=rnd((B, N, 12), f64), g_r_feet=rnd((B, N, 4, 3), f64), g_yaw=rnd((B,), f64),
                 g_pos_des=rnd((B, 3), f64))
    tan = dict(x0=rnd((B, 12), f32), pos_des=rnd((B, 3), f64), cmd=rnd((B, 4), f32),
               foot_lever=rnd((B, 4, 3), f32))
    vres = plan.traj_vjp(*ins, dt, **grads)
    jres = plan.traj_jvp(*ins, dt, tan)
    work = td["pos_des"].clone()                          # the primal clamps it in place
    pres = plan.generate_traj(td["x0"], work, td["cmd"], td["t_now"], td["gait"], td["foot_lever"],
                              td["hip"], dt)
    nbytes = {k: sum(v) for k, v in traffic(N).items()}
    src = {k: torch.empty(B * n, dtype=torch.uint8, device=dev).random_(0, 256)
           for k, n in nbytes.items()}
    dst = {k: torch.empty_like(v) for k, v in src.items()}
    variants = {"vjp": (lambda: plan.traj_vjp(*ins, dt, **grads, out=vres), a.reps),
                "jvp": (lambda: plan.traj_jvp(*ins, dt, tan, out=jres), a.reps),
                "primal": (lambda: plan.generate_traj(td["x0"], work, td["cmd"], td["t_now"],
                                                      td["gait"], td["foot_lever"], td["hip"], dt,
                                                      out=pres), a.reps)}
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
    rec["ratio_vjp_to_primal"] = rec["vjp"]["ms"] / rec["primal"]["ms"]
    rec["ratio_jvp_to_primal"] = rec["jvp"]["ms"] / rec["primal"]["ms"]
    torch.cuda.synchronize(dev)
    rec["nan_robots"] = int(sum(torch.isnan(v.reshape(B, -1)).any(1).sum() for v in vres.values()))
    emit(rec, a.out)


if __name__ == "__main__":
    main()
