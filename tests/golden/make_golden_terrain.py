"""Generate ``tests/golden/qp_terrain.npz``: QPs with a friction coefficient and a stance
normal-force floor of their own (``cmpc_solve_io``'s ``mu`` / ``fz_min``, include/cmpc.h) and
their KKT-certified float64 optima.  Runs on the CPU; needs only ``oracle/`` and ``cmpc.synth``.

Instances (34): the 32 of ``synth.make_batch(32, seed=77, mixed=True)`` plus 2 standing (every
leg in stance over the whole horizon) instances, so that every solve-kernel class is present
(at most 128 free forces, 129..160, more than 160).  Inputs are rounded to fp32, the boundary
type, before anything is solved.

Terrain sets, one value pair per instance:
  A  ``synth.make_terrain(34, seed=5)``: mu ~ U(0.2, 1.0), fz_min ~ U(0, 20)
  B  ``synth.make_terrain(34, seed=6, mu=(0.2, 0.5))``: the tick on which every robot has
     stepped onto ice
For each set the optimum of ``mpc_qp.build_qp(..., mu=mu_i, fz_min=fz_i)`` from
``tight_solver.solve`` in the reference layout (w, lam_x, lam_a) and its certificate (the maximum
KKT residual), which must be <= 1e-8 for every instance.

Usage:  python tests/golden/make_golden_terrain.py
"""
from __future__ import annotations

import multiprocessing as mp
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "convex-mpc-unitree-go2_amd"))

from oracle import mpc_qp, tight_solver  # noqa: E402
from cmpc import synth  # noqa: E402

KEYS = ("Ad", "Bd", "gd", "x0", "xref", "contact")
KKT_BAR = 1e-8


def standing(B: int, seed: int) -> dict:
    """``B`` instances of synth.make_batch(B, seed) (trot) with every leg planted for the whole
    horizon: the planted feet are recovered from the stance steps of the trot (lever = foot -
    com(t), synth.make_batch) and the dynamics rebuilt with synth.discretize."""
    b = synth.make_batch(B, seed, mixed=False)
    N, dt = b["N"], b["dt"]
    t_vec = (np.arange(N) + 1) * dt
    v_des = b["xref"][:, 0, 6:9]
    drift = v_des[:, None, :] * (t_vec - dt)[None, :, None]            # (B, N, 3)
    ct = b["contact"]                                                   # (B, 4, N)
    r_legs = np.zeros((B, N, 4, 3))
    for i in range(B):
        for leg in range(4):
            k = int(np.flatnonzero(ct[i, leg])[0])                      # a step the leg stands in
            r0 = b["r_legs"][i, k, leg] + drift[i, k]
            r_legs[i, :, leg] = r0[None, :] - drift[i]
    Ad, Bd, gd = synth.discretize(b["m"], b["I_world"], r_legs, b["yaw_avg"], dt)
    return dict(Ad=Ad, Bd=Bd, gd=gd, x0=b["x0"], xref=b["xref"],
                contact=np.ones((B, 4, N), np.uint8))


def instances() -> dict:
    a = synth.make_batch(32, seed=77, mixed=True)
    s = standing(2, seed=78)
    out = {k: np.concatenate([a[k], s[k]]) for k in KEYS}
    for k in KEYS[:5]:      # the solver's boundary is fp32: the optimum is that of the rounded QP
        out[k] = out[k].astype(np.float32)
    nf = 3 * (out["contact"] != 0).reshape(34, -1).sum(1)
    classes = np.searchsorted(np.array([128, 160]), nf)               # 0: <= 128, 1: <= 160, 2: 192
    assert all(np.any(classes == c) for c in range(3)), np.bincount(classes, minlength=3)
    return out


def _certify_one(args):
    Ad, Bd, gd, x0, xref, contact, mu, fz = args
    f64 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    qp = mpc_qp.build_qp(f64(Ad), f64(Bd), f64(gd), f64(x0), f64(xref).T, contact,
                         mu=float(mu), fz_min=float(fz))
    r = tight_solver.solve(qp)
    return r["w"], r["lam_x"], r["lam_a"], max(r["kkt"].values())


def certify(batch, terrain):
    jobs = [tuple(batch[k][i] for k in KEYS) + (terrain["mu"][i], terrain["fz_min"][i])
            for i in range(len(terrain["mu"]))]
    with mp.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(_certify_one, jobs, chunksize=1)
    W, LX, LA, K = (np.array(x) for x in zip(*res))
    assert K.max() <= KKT_BAR, (K.max(), np.flatnonzero(K > KKT_BAR))
    return W, LX, LA, K


def main(name: str = "qp_terrain.npz"):
    batch = instances()
    tA = synth.make_terrain(34, seed=5)
    tB = synth.make_terrain(34, seed=6, mu=(0.2, 0.5))
    out = dict(batch)
    for tag, t in (("A", tA), ("B", tB)):
        W, LX, LA, K = certify(batch, t)
        out.update({f"mu_{tag}": t["mu"].astype(np.float32),
                    f"fz_min_{tag}": t["fz_min"].astype(np.float32),
                    f"w_{tag}": W, f"lam_x_{tag}": LX, f"lam_a_{tag}": LA, f"kkt_{tag}": K})
        print(f"set {tag}: max KKT {K.max():.2e}")
    np.savez_compressed(HERE / name, **out)
    print(name, (HERE / name).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
