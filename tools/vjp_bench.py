"""What the backward pass costs: Plan.vjp on config 3 (65,536 QPs) for the gradients in x0 and
xref and for every output, next to Plan.gain for K alone and for every output, to a
device-to-device copy of the bytes each reads and writes and to a cold and a warm solve step of
the same batch, all in one process.

The faces are read off the batch's own solve (w_out); gw is a fixed random fp32 array.  Each
round times the variants one after the other with HIP events (--reps launches per event pair for
the short ones), after --warmup untimed rounds; the record holds the median and the min / max
over --rounds rounds, the bytes per instance and the ratios.  The condition the design is held
to: vjp with every output costs less than two gain launches with every output (running the
recursion twice is what the shared column avoids).
   usage: python tools/vjp_bench.py [--batch 65536] [--rounds 10] [--warmup 3] [--reps 5]
                                    [--out profiles/vjp_bench.json]"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "convex-mpc-unitree-go2_amd"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

from cmpc import Plan, SolverParams, _lib, synth, to_device_batch  # noqa: E402

from bench_util import emit, interleaved_rounds  # noqa: E402
from gain_bench import ALL as GAIN_ALL, bytes_moved as gain_bytes  # noqa: E402

VJP_ALL = _lib.VJP_OUTPUTS
VJP_WORDS = dict(x0=12, gd=12, Q=12, R=12, mu=1, fz_min=1, Ad=144)   # fp64 words, N apart


def vjp_bytes(N, want):
    """Bytes cmpc_vjp_run reads and writes per instance: Ad, Bd, gd, x0, xref, w's forces, gw
    (fp32), contact; the wanted gradients (fp64)."""
    rd = 4 * (144 + 144 * N + 12 + 12 + 12 * N + 12 * N + 24 * N) + 4 * N
    wr = 8 * sum(12 * N if n == "xref" else 144 * N if n == "Bd" else VJP_WORDS[n] for n in want)
    return rd, wr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=str(REPO / "profiles" / "vjp_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vjp_bench: no ROCm device (nothing is measured without one)")
    B = a.batch
    plan = Plan(SolverParams(max_batch=B))
    N = plan.params.N
    dev = plan.device
    d = to_device_batch(synth.make_config(3, B=B), dev)
    args = [d[k] for k in ("Ad", "Bd", "gd", "x0", "xref", "contact")]
    y = torch.zeros((B, 12 * N), dtype=torch.float32, device=dev)
    w, st, it = plan.solve(*args, y_out=y)
    out = (torch.empty_like(w), torch.empty_like(st), torch.empty_like(it))
    y2 = torch.empty_like(y)
    gw = torch.randn((B, 24 * N), dtype=torch.float32, device=dev,
                     generator=torch.Generator(device=dev).manual_seed(5))
    gres = plan.gain(*args, w=w, want=GAIN_ALL)
    vres = plan.vjp(*args, gw, w=w, want=VJP_ALL)
    vmodes = {"x0_xref": ("x0", "xref"), "all": VJP_ALL}
    gmodes = {"K": ("K",), "all": GAIN_ALL}
    nbytes = {"vjp_" + m: sum(vjp_bytes(N, v)) for m, v in vmodes.items()}
    nbytes.update({"gain_" + m: sum(gain_bytes(N, m == "all")) for m in gmodes})
    src = {m: torch.empty(B * n, dtype=torch.uint8, device=dev).random_(0, 256)
           for m, n in nbytes.items()}
    dst = {m: torch.empty_like(v) for m, v in src.items()}
    variants = {}
    for m, v in vmodes.items():
        variants["vjp_" + m] = (lambda v=v: plan.vjp(*args, gw, w=w, want=v, out=vres), a.reps)
    for m, v in gmodes.items():
        variants["gain_" + m] = (lambda v=v: plan.gain(*args, w=w, want=v, out=gres), a.reps)
    for m in nbytes:
        variants["copy_" + m] = (lambda m=m: dst[m].copy_(src[m]), a.reps)
    variants["solve_cold"] = (lambda: plan.solve(*args, out=out), 1)
    variants["solve_warm"] = (lambda: plan.solve(*args, out=out, w_init=w, y_init=y, y_out=y2), 1)
    rec = {"config": 3, "batch": B, "N": N, "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(dev)}
    rec.update(interleaved_rounds(variants, a.warmup, a.rounds))
    for m in nbytes:
        k = rec[m]
        rd, wr = (vjp_bytes(N, vmodes[m[4:]]) if m.startswith("vjp_") else
                  gain_bytes(N, m == "gain_all"))
        k["bytes_read_per_instance"], k["bytes_written_per_instance"] = rd, wr
        k["ratio_to_copy"] = k["ms"] / rec["copy_" + m]["ms"]
        k["ratio_to_solve_cold"] = k["ms"] / rec["solve_cold"]["ms"]
        k["ratio_to_solve_warm"] = k["ms"] / rec["solve_warm"]["ms"]
        rec["copy_" + m]["bytes"] = 2 * nbytes[m] * B     # a copy reads and writes each byte
    two = 2.0 * rec["gain_all"]["ms"]
    rec["condition"] = {"vjp_all_ms": rec["vjp_all"]["ms"], "two_gain_all_ms": two,
                        "vjp_all_over_two_gain_all": rec["vjp_all"]["ms"] / two,
                        "holds": bool(rec["vjp_all"]["ms"] < two)}
    vres = plan.vjp(*args, gw, w=w, want=VJP_ALL)
    torch.cuda.synchronize(dev)
    rec["status1"] = int((st == 1).sum())
    rec["nan_instances"] = int(torch.isnan(vres["x0"]).any(1).sum())
    emit(rec, a.out)


if __name__ == "__main__":
    main()
