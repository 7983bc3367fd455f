"""What the *_bench.py tools share: HIP-event timing, the interleaved-rounds protocol and its
summary (kkt_bench, gain_bench), the timed cold solve steps of one batch (terrain_bench,
weights_bench), and the one-line JSON record."""
import json
from pathlib import Path

import numpy as np
import torch


def timed(fn, reps):
    """ms per call of fn over reps launches between one pair of HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def summary(ms):
    return {"ms": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def interleaved_rounds(variants, warmup, rounds):
    """variants: name -> (fn, reps).  Each round times the variants one after the other; the
    first ``warmup`` rounds are dropped.  -> name -> summary of the ``rounds`` kept."""
    ms = {k: [] for k in variants}
    for r in range(warmup + rounds):
        for k, (fn, reps) in variants.items():
            t = timed(fn, reps)
            if r >= warmup:
                ms[k].append(t)
    return {k: summary(v) for k, v in ms.items()}


def solve_steps(plan, d, steps, warmup, **kw):
    """``steps`` timed cold solves of the device batch d after ``warmup`` untimed ones: ms per
    step, the status histogram and the mean / max ADMM iterations."""
    B = d["Ad"].shape[0]
    N = plan.params.N
    out = (torch.empty((B, 24 * N), dtype=torch.float32, device=plan.device),
           torch.empty((B,), dtype=torch.int32, device=plan.device),
           torch.empty((B,), dtype=torch.int32, device=plan.device))
    step = lambda: plan.solve(d["Ad"], d["Bd"], d["gd"], d["x0"], d["xref"], d["contact"],  # noqa: E731
                              out=out, **kw)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(plan.device)
    t = summary([timed(step, 1) for _ in range(steps)])
    st, it = out[1].cpu().numpy(), out[2].cpu().numpy()
    vals, cnt = np.unique(st, return_counts=True)
    return {"ms_per_step": t["ms"], "ms_min": t["ms_min"], "ms_max": t["ms_max"],
            "status": {str(int(v)): int(c) for v, c in zip(vals, cnt)},
            "iters_mean": float(it.mean()), "iters_max": int(it.max())}


def emit(rec, out):
    """Print the record as one JSON line and, with ``out``, write it there."""
    line = json.dumps(rec)
    print(line)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(line + "\n")
