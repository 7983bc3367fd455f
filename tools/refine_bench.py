"""What the certified float64 refinement costs and what it finds: Plan.refine on config 3
(65,536 QPs), on the cold solve's answers and on the next tick's warm ones, next to a cold solve
step and a Plan.gain launch with u_star of the same batch, all in one process.

Each batch is solved with default parameters and refined in place (w_out = w, status in/out)
with max_rounds = 8.  The record holds, per batch: the histogram of info; the share of the
status-1 and of the status-2 answers that were certified; over the certified status-1 answers
the distribution of res[2], the measured distance of the fp32 answer from the float64 optimum
(max, median, the counts above 1e-4 and above 5e-5) -- the parity survey, on the device; and the
certified share when the faces are read off the solver's answers with face_tol 1e-6 (the one
used), 1e-5 and 1e-4.  A third batch gets the same survey without timing: the fresh-seed warm
tick of tests/test_gpu_warm.py, whose two status-1 answers above 1e-4 are reported one by one
(known_misses).  Timing: each round times the variants one after the other with HIP events
(--reps launches per event pair for the short ones) after --warmup untimed rounds; the timed
refine launches read the solve's untouched answers and write a separate w_out, the same work as
the in-place call.
   usage: python tools/refine_bench.py [--batch 65536] [--rounds 10] [--warmup 3] [--reps 3]
                                       [--out profiles/refine_bench.json]"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "convex-mpc-unitree-go2_amd"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

from cmpc import Plan, SolverParams, synth, to_device_batch  # noqa: E402

from bench_util import emit, interleaved_rounds  # noqa: E402

FACE_TOLS = (1e-6, 1e-5, 1e-4)
KEYS = ("Ad", "Bd", "gd", "x0", "xref", "contact")
FRESH_IDS = (31439, 5794)   # tests/test_gpu_warm.py: accepted 2.1e-4 / 1.1e-4 off at status 1


def hist(t):
    vals, cnt = torch.unique(t, return_counts=True)
    return {str(int(v)): int(c) for v, c in zip(vals.cpu(), cnt.cpu())}


def survey(plan, args, w, st, max_rounds):
    """Refine copies of (w, st) in place -> the record of one batch."""
    rec = {"status_in": hist(st), "face_tol": FACE_TOLS[0], "max_rounds": max_rounds}
    by_tol = {}
    for tol in FACE_TOLS:
        w2, st2 = w.clone(), st.clone()
        out = plan.refine(*args, w=w2, w_out=w2, status=st2, face_tol=tol, max_rounds=max_rounds)
        torch.cuda.synchronize(plan.device)
        info, res = out["info"], out["res"]
        cert = info >= 0
        share = {f"status{s}": {"count": int((st == s).sum()), "certified": int((cert & (st == s)).sum())}
                 for s in (1, 2)}
        by_tol[f"{tol:g}"] = {"certified": int(cert.sum()), **share}
        if tol != FACE_TOLS[0]:
            continue
        rec["info"] = hist(info)
        rec["certified"] = int(cert.sum())
        rec["certified_share"] = share
        rec["rows_untouched_when_not_certified"] = bool(torch.equal(w2[~cert], w[~cert]) and
                                                        torch.equal(st2[~cert], st[~cert]))
        rec["status_out"] = hist(st2)
        d = res[cert & (st == 1), 2]
        rec["res2_certified_status1"] = {
            "count": int(d.numel()), "max": float(d.max()), "median": float(d.median()),
            "above_1e-4": int((d > 1e-4).sum()), "above_5e-5": int((d > 5e-5).sum())}
        d2 = res[cert & (st == 2), 2]
        if d2.numel():
            rec["res2_certified_status2"] = {"count": int(d2.numel()), "max": float(d2.max()),
                                             "above_1e-4": int((d2 > 1e-4).sum())}
        rec["repaired_share_of_certified"] = float((info > 0).sum()) / max(1, int(cert.sum()))
    rec["by_face_tol"] = by_tol
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-rounds", type=int, default=8)
    ap.add_argument("--out", type=str, default=str(REPO / "profiles" / "refine_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("refine_bench: no ROCm device (nothing is measured without one)")
    B = a.batch
    plan = Plan(SolverParams(max_batch=B))
    N = plan.params.N
    dev = plan.device
    b0 = synth.make_config(3, B=B)
    d0, d1 = to_device_batch(b0, dev), to_device_batch(synth.next_tick(b0), dev)
    args0, args1 = [d0[k] for k in KEYS], [d1[k] for k in KEYS]
    y = torch.zeros((B, 12 * N), dtype=torch.float32, device=dev)
    w0, st0, _ = plan.solve(*args0, y_out=y)
    w1, st1, _ = plan.solve(*args1, w_init=w0, y_init=y)
    torch.cuda.synchronize(dev)
    rec = {"config": 3, "batch": B, "N": N, "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(dev),
           "cold": survey(plan, args0, w0, st0, a.max_rounds),
           "warm_next_tick": survey(plan, args1, w1, st1, a.max_rounds)}
    # the fresh-seed warm tick of tests/test_gpu_warm.py (the status-1 hole), with
    # what the refinement makes of its two known misses
    bp = synth.make_batch(B, 13, mixed=True)
    dp, dn = to_device_batch(bp, dev), to_device_batch(synth.next_tick(bp), dev)
    argsn = [dn[k] for k in KEYS]
    wp, _, _ = plan.solve(*[dp[k] for k in KEYS], y_out=y)
    wn, stn, _ = plan.solve(*argsn, w_init=wp, y_init=y)
    torch.cuda.synchronize(dev)
    rec["fresh_seed_warm"] = survey(plan, argsn, wn, stn, a.max_rounds)
    ids = [i for i in FRESH_IDS if i < B]
    if ids:
        r = plan.refine(*[t[ids] for t in argsn], w=wn[ids], max_rounds=a.max_rounds)
        torch.cuda.synchronize(dev)
        rec["fresh_seed_warm"]["known_misses"] = {
            "ids": ids, "status_in": stn[ids].tolist(), "info": r["info"].tolist(),
            "res2": r["res"][:, 2].tolist()}
    del dp, dn, wp
    out = (torch.empty_like(w0), torch.empty_like(st0), torch.empty_like(st0))
    w_buf, st_buf = torch.empty_like(w0), torch.empty_like(st0)
    r_out = {"info": torch.empty(B, dtype=torch.int32, device=dev),
             "res": torch.empty((B, 3), dtype=torch.float64, device=dev)}
    g_out = plan.gain(*args0, w=w0, want=("K", "u_star"))
    variants = {
        "refine_cold": (lambda: plan.refine(*args0, w=w0, w_out=w_buf, status=st_buf,
                                            max_rounds=a.max_rounds, out=r_out), a.reps),
        "refine_warm": (lambda: plan.refine(*args1, w=w1, w_out=w_buf, status=st_buf,
                                            max_rounds=a.max_rounds, out=r_out), a.reps),
        "refine_check_only": (lambda: plan.refine(*args0, w=w0, w_out=w_buf, status=st_buf,
                                                  max_rounds=0, out=r_out), a.reps),
        "gain_u_star": (lambda: plan.gain(*args0, w=w0, want=("K", "u_star"), out=g_out), a.reps),
        "solve_cold": (lambda: plan.solve(*args0, out=out), 1),
    }
    rec.update(interleaved_rounds(variants, a.warmup, a.rounds))
    for k in ("refine_cold", "refine_warm", "refine_check_only"):
        rec[k]["ratio_to_solve_cold"] = rec[k]["ms"] / rec["solve_cold"]["ms"]
        rec[k]["ratio_to_gain_u_star"] = rec[k]["ms"] / rec["gain_u_star"]["ms"]
    emit(rec, a.out)


if __name__ == "__main__":
    main()
