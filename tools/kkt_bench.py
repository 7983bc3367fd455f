"""What the device-side KKT evaluation costs: Plan.kkt on config 3 (65,536 QPs) in both modes
(multipliers given / recovered on the device), against a device-to-device copy of the number of
bytes the kernel reads and against one cold solve step of the same batch, all in one process.

The evaluated points are the batch's own solve (w and lam_out).  Each round times the variants
one after the other with HIP events (--reps launches per event pair for the short ones), after
--warmup untimed rounds; the record holds the median and the min / max over --rounds rounds,
the bytes per instance, the achieved read rate, the two ratios, and the residuals the
evaluation reports for the batch (largest stat / prim / comp over status-1 answers per mode).
   usage: python tools/kkt_bench.py [--batch 65536] [--rounds 10] [--warmup 3] [--reps 20]
                                    [--out profiles/kkt_bench.json]"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "convex-mpc-unitree-go2_amd"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cmpc import KKT_COLUMNS, Plan, SolverParams, synth, to_device_batch  # noqa: E402

from bench_util import emit, interleaved_rounds  # noqa: E402


def bytes_read(N, with_lam):
    """Bytes cmpc_kkt_run reads per instance: Ad, Bd, gd, x0, xref (fp32), contact, w (+ lam)."""
    return 4 * (144 + 144 * N + 12 + 12 + 12 * N + 24 * N + (52 * N if with_lam else 0)) + 4 * N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=str(REPO / "profiles" / "kkt_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kkt_bench: no ROCm device (nothing is measured without one)")
    B = a.batch
    plan = Plan(SolverParams(max_batch=B))
    N = plan.params.N
    dev = plan.device
    d = to_device_batch(synth.make_config(3, B=B), dev)
    args = [d[k] for k in ("Ad", "Bd", "gd", "x0", "xref", "contact")]
    w, st, it, lam = plan.solve(*args, lam_out=True)
    out = (torch.empty_like(w), torch.empty_like(st), torch.empty_like(it))
    res = torch.empty((B, 4), dtype=torch.float64, device=dev)
    nbytes = {m: bytes_read(N, m == "given") for m in ("given", "recovered")}
    src = {m: torch.empty(B * n, dtype=torch.uint8, device=dev).random_(0, 256)
           for m, n in nbytes.items()}
    dst = {m: torch.empty_like(v) for m, v in src.items()}
    variants = {
        "kkt_given": (lambda: plan.kkt(*args, w, lam=lam, out=res), a.reps),
        "kkt_recovered": (lambda: plan.kkt(*args, w, out=res), a.reps),
        "copy_given": (lambda: dst["given"].copy_(src["given"]), a.reps),
        "copy_recovered": (lambda: dst["recovered"].copy_(src["recovered"]), a.reps),
        "solve_cold": (lambda: plan.solve(*args, out=out), 1),
    }
    rec = {"config": 3, "batch": B, "N": N, "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(dev), "columns": list(KKT_COLUMNS)}
    rec.update(interleaved_rounds(variants, a.warmup, a.rounds))
    ok = (st == 1).cpu().numpy()
    rec["status1"] = int(ok.sum())
    for m in ("given", "recovered"):
        k = rec["kkt_" + m]
        k["bytes_read_per_instance"] = nbytes[m]
        k["read_GB_per_s"] = nbytes[m] * B / (k["ms"] * 1e-3) / 1e9
        k["ratio_to_copy"] = k["ms"] / rec["copy_" + m]["ms"]
        k["ratio_to_solve"] = k["ms"] / rec["solve_cold"]["ms"]
        rec["copy_" + m]["bytes"] = nbytes[m] * B
        v = plan.kkt(*args, w, lam=lam if m == "given" else None).cpu().numpy()
        k["status1_max"] = {c: float(v[ok, i].max()) for i, c in enumerate(KKT_COLUMNS) if i}
        k["status1_inf_comp"] = int(np.isinf(v[ok, 3]).sum())
    emit(rec, a.out)


if __name__ == "__main__":
    main()
