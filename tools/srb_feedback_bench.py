"""What the plant's inner-loop force feedback costs and what it does to a pushed robot.

Timing (HIP events, one process): at --batch robots and --nsub substeps, Plan.srb_step plain,
with the law (K, x_solve, contact, mu, fz_min), with the law and a wrench, and with both outputs
too, next to a device-to-device copy of the bytes each variant reads and writes (a copy of n bytes
reads n and writes n: it moves twice the bytes of the entry it stands next to, the convention of
srb_grad_bench.py).  The robots, forces and gains are those of a ClosedLoop(feedback=True) after a
few ticks; before every timed window the state is put back to that snapshot (untimed), so the
plant never runs away from the solve it holds.  The comparison value of the issue is plain + copy.
Then the graph-replayed ClosedLoop tick with gain=True against feedback=True, interleaved, at
--batch and at --small robots.

Push recovery: --push-batch robots trot forward at 0.5 m/s with random headings; at tick
--push-tick a lateral (body-y) force of each of --pushes newtons is held for one tick, with
feedback off and on.  Each run is compared with its twin, the same robots never pushed: the peak
difference in lateral body velocity and in roll after the push, the ticks until a robot is back
for good within its pre-push band (the half range of the twin's own signal, the gait's ripple,
over the --band ticks before the push), the COM height excursion and, with feedback, the share of
fb_status 2 after the push.
   usage: python tools/srb_feedback_bench.py [--batch 65536] [--small 1024] [--nsub 20]
              [--rounds 10] [--warmup 3] [--reps 5] [--out profiles/srb_feedback_bench.json]"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "convex-mpc-unitree-go2_amd"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cmpc import Plan, SolverParams  # noqa: E402
from cmpc.closed_loop import ClosedLoop  # noqa: E402

from bench_util import emit, summary, timed  # noqa: E402

# bytes per robot: t_now, gait fp64; mass, inertia, force, x, feet fp32; contact_state in and out
PLAIN = (8 * (1 + 6) + 4 * (1 + 9 + 12 + 12 + 12) + 1, 4 * 24 + 1)
LAW = 8 * 144 + 4 * 12 + 4 + 4 * 2       # K, x_solve, contact[:, :, 0], mu, fz_min
TRAFFIC = {"plain": PLAIN, "law": (PLAIN[0] + LAW, PLAIN[1]),
           "law_wrench": (PLAIN[0] + LAW + 24, PLAIN[1]),
           "all": (PLAIN[0] + LAW + 24, PLAIN[1] + 48 + 1)}


def _command(B, vx=0.5):
    cmd = np.zeros((B, 4))
    cmd[:, 0], cmd[:, 2] = vx, 0.27
    return cmd


def step_times(plan, B, nsub, a):
    dev = plan.device
    cl = ClosedLoop(B, plan=plan, seed=1, nsub=nsub, feedback=True, push=True,
                    mu=np.full(B, 0.8), fz_min=np.full(B, 10.0))
    cl.set_command(_command(B))
    for _ in range(6):
        cl.tick()
    N = cl.N
    snap = (cl.x.clone(), cl.feet.clone(), cl.contact.clone())
    x, feet, cs = (t.clone() for t in snap)
    force_out = torch.empty((B, 12), dtype=torch.float32, device=dev)
    status = torch.empty((B,), dtype=torch.uint8, device=dev)
    wrench = torch.zeros((B, 6), dtype=torch.float32, device=dev)
    wrench[:, 1] = 30.0
    base = (cl.t, cl.gait, cl.mass, cl.I_body, cl.w[:, 12 * N:], cl.hip, x, feet, cs, nsub,
            cl.dt / nsub)
    law = dict(K=cl.K0, x_solve=cl.x_solve, contact=cl.ct, mu=cl.mu, fz_min=cl.fz_min)
    calls = {"plain": lambda: plan.srb_step(*base),
             "law": lambda: plan.srb_step(*base, **law),
             "law_wrench": lambda: plan.srb_step(*base, **law, wrench=wrench),
             "all": lambda: plan.srb_step(*base, **law, wrench=wrench, force_out=force_out,
                                          fb_status=status)}
    nbytes = {k: sum(v) for k, v in TRAFFIC.items()}
    src = {k: torch.empty(B * n, dtype=torch.uint8, device=dev).random_(0, 256)
           for k, n in nbytes.items()}
    dst = {k: torch.empty_like(v) for k, v in src.items()}
    for k in nbytes:
        calls["copy_" + k] = lambda k=k: dst[k].copy_(src[k])
    ms = {k: [] for k in calls}
    for r in range(a.warmup + a.rounds):
        for k, fn in calls.items():
            for t, s in zip((x, feet, cs), snap):
                t.copy_(s)
            v = timed(fn, a.reps)
            if r >= a.warmup:
                ms[k].append(v)
    rec = {"batch": B, "nsub": nsub}
    rec.update({k: summary(v) for k, v in ms.items()})
    for k, (rd, wr) in TRAFFIC.items():
        rec[k]["bytes_read_per_robot"], rec[k]["bytes_written_per_robot"] = rd, wr
        rec[k]["ratio_to_copy"] = rec[k]["ms"] / rec["copy_" + k]["ms"]
        rec["copy_" + k]["bytes"] = 2 * nbytes[k] * B
        if k != "plain":
            rec[k]["ratio_to_plain_plus_copy"] = rec[k]["ms"] / (rec["plain"]["ms"]
                                                                 + rec["copy_" + k]["ms"])
    torch.cuda.synchronize(dev)
    st = status.cpu().numpy()
    rec["fb_status_share"] = [float(np.mean(st == s)) for s in (0, 1, 2)]
    rec["finite"] = bool(torch.isfinite(x).all())
    return rec


def tick_times(plan, B, nsub, a):
    loops = {}
    for name, kw in (("gain", dict(gain=True)), ("feedback", dict(feedback=True))):
        cl = ClosedLoop(B, plan=plan, seed=1, nsub=nsub, **kw)
        cl.set_command(_command(B))
        for _ in range(4):
            cl.tick()
        cl.capture()
        loops[name] = cl
    ms = {k: [] for k in loops}
    for r in range(a.warmup + a.rounds):
        for k, cl in loops.items():
            v = timed(cl.tick, a.reps)
            if r >= a.warmup:
                ms[k].append(v)
    rec = {"batch": B, "nsub": nsub}
    rec.update({k: summary(v) for k, v in ms.items()})
    rec["feedback_over_gain"] = rec["feedback"]["ms"] / rec["gain"]["ms"]
    rec["solved"] = {k: float((cl.status == 1).float().mean()) for k, cl in loops.items()}
    return rec


def walk(plan, B, push, feedback, a):
    """One run: per tick the lateral body velocity, roll, height and fb_status == 2 of every
    robot."""
    cl = ClosedLoop(B, plan=plan, seed=2, feedback=feedback, push=True)
    cl.set_command(_command(B))
    ticks = a.push_tick + 1 + a.after
    vy, roll, z, clamped = (np.zeros((ticks, B)) for _ in range(4))
    for k in range(ticks):
        if k == a.push_tick:                       # body-y, in the world frame at the push
            yaw = cl.x[:, 5]
            cl.wrench[:, 0], cl.wrench[:, 1] = -push * yaw.sin(), push * yaw.cos()
        elif k == a.push_tick + 1:
            cl.wrench.zero_()
        cl.tick()
        x = cl.x.cpu().numpy().astype(np.float64)
        vy[k] = -np.sin(x[:, 5]) * x[:, 6] + np.cos(x[:, 5]) * x[:, 7]
        roll[k], z[k] = x[:, 3], x[:, 2]
        if feedback:
            clamped[k] = cl.fb_status.cpu().numpy() == 2
    return dict(lateral_velocity=vy, roll=roll, height=z, clamped=clamped)


def push_run(plan, B, push, feedback, a, twin):
    """The pushed run against ``twin``, the same robots never pushed: the deviation is the
    difference of the two, and a robot's band is the half range of the twin's own signal (the
    gait's ripple) over the --band ticks before the push."""
    run = walk(plan, B, push, feedback, a)
    pre = slice(a.push_tick - a.band, a.push_tick)
    rec = {"push_N": push, "feedback": feedback,
           "fallen_or_nonfinite": float(np.mean(~np.isfinite(run["height"][-1])
                                                | (run["height"][-1] < 0.15)))}
    for name in ("lateral_velocity", "roll"):
        dev = np.abs(run[name] - twin[name])[a.push_tick:]
        band = (twin[name][pre].max(0) - twin[name][pre].min(0)) / 2
        out = dev > band
        last = np.where(out.any(0), out.shape[0] - out[::-1].argmax(0), 0)
        rec[name] = {"peak_mean": float(dev.max(0).mean()), "peak_max": float(dev.max()),
                     "band_mean": float(band.mean()),
                     "ticks_back_median": float(np.median(last)),
                     "ticks_back_p95": float(np.percentile(last, 95)),
                     "never_back_share": float(np.mean(last >= out.shape[0]))}
    dz = np.abs(run["height"] - twin["height"])[a.push_tick:].max(0)
    rec["height_excursion"] = {"mean": float(dz.mean()), "max": float(dz.max())}
    if feedback:
        rec["fb_status_2_share_after_push"] = float(run["clamped"][a.push_tick:].mean())
        rec["fb_status_2_share_unpushed"] = float(twin["clamped"][a.push_tick:].mean())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--small", type=int, default=1024)
    ap.add_argument("--nsub", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--push-batch", type=int, default=4096)
    ap.add_argument("--push-tick", type=int, default=24)
    ap.add_argument("--band", type=int, default=12)
    ap.add_argument("--after", type=int, default=72)
    ap.add_argument("--pushes", type=str, default="30,60,120")
    ap.add_argument("--out", type=str, default=str(REPO / "profiles" / "srb_feedback_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("srb_feedback_bench: no ROCm device (nothing is measured without one)")
    plan = Plan(SolverParams(max_batch=max(a.batch, a.small, a.push_batch)))
    twins = {fb: walk(plan, a.push_batch, 0.0, fb, a) for fb in (False, True)}
    rec = {"N": plan.params.N, "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(plan.device),
           "step": step_times(plan, a.batch, a.nsub, a),
           "tick": [tick_times(plan, B, a.nsub, a) for B in (a.batch, a.small)],
           "push": [push_run(plan, a.push_batch, float(f), fb, a, twins[fb])
                    for f in a.pushes.split(",") for fb in (False, True)]}
    emit(rec, a.out)


if __name__ == "__main__":
    main()
