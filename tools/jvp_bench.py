"""What forward mode costs: Plan.jvp on config 3 (65,536 QPs) with d_x0 alone and with all nine
tangents, next to Plan.vjp with all nine outputs, Plan.gain with every output and a
device-to-device copy of the bytes each jvp reads and writes, all in one process.

The faces are read off the batch's own solve (w_out); the tangents and gw are fixed random fp32
arrays.  Each round times the variants one after the other with HIP events (--reps launches per
event pair), after --warmup untimed rounds; the record holds the median and the min / max over
--rounds rounds, the bytes per instance and the ratios.  There is no time bar; the comparison
recorded is one all-nine jvp launch against two gain launches with every output, the central
difference it replaces.
   usage: python tools/jvp_bench.py [--batch 65536] [--rounds 10] [--warmup 3] [--reps 5]
                                    [--out profiles/jvp_bench.json]"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "convex-mpc-unitree-go2_amd"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

from cmpc import Plan, SolverParams, _lib, synth, to_device_batch  # noqa: E402

from bench_util import emit, interleaved_rounds  # noqa: E402
from gain_bench import ALL as GAIN_ALL  # noqa: E402

JVP_ALL = _lib.JVP_TANGENTS
VJP_ALL = _lib.VJP_OUTPUTS
WORDS = dict(x0=12, gd=12, Q=12, R=12, mu=1, fz_min=1, Ad=144)   # fp32 words, N apart


def jvp_bytes(N, names):
    """Bytes cmpc_jvp_run reads and writes per instance: Ad, Bd, gd, x0, xref, w's forces (fp32),
    contact, the given tangents (fp32); dw (fp64)."""
    rd = 4 * (144 + 144 * N + 12 + 12 + 12 * N + 12 * N) + 4 * N
    rd += 4 * sum(12 * N if n == "xref" else 144 * N if n == "Bd" else WORDS[n] for n in names)
    return rd, 8 * 24 * N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=str(REPO / "profiles" / "jvp_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jvp_bench: no ROCm device (nothing is measured without one)")
    B = a.batch
    plan = Plan(SolverParams(max_batch=B))
    N = plan.params.N
    dev = plan.device
    d = to_device_batch(synth.make_config(3, B=B), dev)
    args = [d[k] for k in ("Ad", "Bd", "gd", "x0", "xref", "contact")]
    w, st, it = plan.solve(*args)
    gen = torch.Generator(device=dev).manual_seed(5)
    shapes = dict(x0=(B, 12), xref=(B, N, 12), gd=(B, 12), Q=(B, 12), R=(B, 12), mu=(B,),
                  fz_min=(B,), Ad=(B, 12, 12), Bd=(B, N, 12, 12))
    tan = {n: torch.randn(s, dtype=torch.float32, device=dev, generator=gen)
           for n, s in shapes.items()}
    gw = torch.randn((B, 24 * N), dtype=torch.float32, device=dev, generator=gen)
    dw = plan.jvp(*args, tan, w=w)
    gres = plan.gain(*args, w=w, want=GAIN_ALL)
    vres = plan.vjp(*args, gw, w=w, want=VJP_ALL)
    jmodes = {"x0": ("x0",), "all": JVP_ALL}
    nbytes = {"jvp_" + m: sum(jvp_bytes(N, v)) for m, v in jmodes.items()}
    src = {m: torch.empty(B * n, dtype=torch.uint8, device=dev).random_(0, 256)
           for m, n in nbytes.items()}
    dst = {m: torch.empty_like(v) for m, v in src.items()}
    variants = {}
    for m, v in jmodes.items():
        sub = {n: tan[n] for n in v}
        variants["jvp_" + m] = (lambda sub=sub: plan.jvp(*args, sub, w=w, out=dw), a.reps)
    variants["vjp_all"] = (lambda: plan.vjp(*args, gw, w=w, want=VJP_ALL, out=vres), a.reps)
    variants["gain_all"] = (lambda: plan.gain(*args, w=w, want=GAIN_ALL, out=gres), a.reps)
    for m in nbytes:
        variants["copy_" + m] = (lambda m=m: dst[m].copy_(src[m]), a.reps)
    rec = {"config": 3, "batch": B, "N": N, "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(dev)}
    rec.update(interleaved_rounds(variants, a.warmup, a.rounds))
    for m, v in jmodes.items():
        k = rec["jvp_" + m]
        k["bytes_read_per_instance"], k["bytes_written_per_instance"] = jvp_bytes(N, v)
        k["ratio_to_copy"] = k["ms"] / rec["copy_jvp_" + m]["ms"]
        k["ratio_to_gain_all"] = k["ms"] / rec["gain_all"]["ms"]
        k["ratio_to_vjp_all"] = k["ms"] / rec["vjp_all"]["ms"]
        rec["copy_jvp_" + m]["bytes"] = 2 * nbytes["jvp_" + m] * B   # a copy reads and writes each byte
    two = 2.0 * rec["gain_all"]["ms"]
    rec["comparison"] = {"jvp_all_ms": rec["jvp_all"]["ms"], "two_gain_all_ms": two,
                         "jvp_all_over_two_gain_all": rec["jvp_all"]["ms"] / two}
    dw = plan.jvp(*args, tan, w=w)
    torch.cuda.synchronize(dev)
    rec["status1"] = int((st == 1).sum())
    rec["nan_instances"] = int(torch.isnan(dw).any(1).sum())
    emit(rec, a.out)


if __name__ == "__main__":
    main()
