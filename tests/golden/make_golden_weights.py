"""Generate ``tests/golden/qp_weights.npz``: QPs with cost weights of their own
(``cmpc_solve_io``'s ``Q`` / ``R``, include/cmpc.h) and their KKT-certified float64 optima.  Runs
on the CPU; needs only ``oracle/``, ``cmpc.synth`` and ``tests/golden/qp_terrain.npz``.

Instances (34): the inputs of ``qp_terrain.npz`` (make_golden_terrain.py: every solve-kernel
class, two instances above 160 free forces), already rounded to fp32.  The plan's mu = 0.8 and
fz_min = 10 serve every instance.

Weight sets, one (Q, R) row pair per instance:
  A  ``synth.make_weights(34, seed=21)``: Q = default x exp(U(-ln 4, ln 4)) per entry, drawn
     first, then R log-uniform in [2.5e-6, 1e-4]
  B  ``synth.make_weights(34, seed=22, q_span=10, r=(1e-6, 1e-3))``, then ``Q[::5, 0] = 0`` and
     ``Q[1::5, 5] = 0``: a wider draw with unweighted states
For each set the optimum of ``mpc_qp.build_qp(..., Q=Q_i, R=R_i)`` from ``tight_solver.solve`` in
the reference layout (w, lam_x, lam_a) and its certificate (the maximum KKT residual), which must
be <= 1e-8 for every instance.

Usage:  python tests/golden/make_golden_weights.py
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
MU, FZ_MIN = 0.8, 10.0


def weight_sets() -> dict:
    A = synth.make_weights(34, seed=21)
    B = synth.make_weights(34, seed=22, q_span=10.0, r=(1e-6, 1e-3))
    B["Q"][::5, 0] = 0.0
    B["Q"][1::5, 5] = 0.0
    return {"A": A, "B": B}


def _certify_one(args):
    Ad, Bd, gd, x0, xref, contact, Q, R = args
    f64 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    qp = mpc_qp.build_qp(f64(Ad), f64(Bd), f64(gd), f64(x0), f64(xref).T, contact,
                         Q=f64(Q), R=f64(R), mu=MU, fz_min=FZ_MIN)
    r = tight_solver.solve(qp)
    return r["w"], r["lam_x"], r["lam_a"], max(r["kkt"].values())


def certify(batch, wt):
    jobs = [tuple(batch[k][i] for k in KEYS) + (wt["Q"][i], wt["R"][i]) for i in range(len(wt["Q"]))]
    with mp.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(_certify_one, jobs, chunksize=1)
    W, LX, LA, K = (np.array(x) for x in zip(*res))
    assert K.max() <= KKT_BAR, (K.max(), np.flatnonzero(K > KKT_BAR))
    return W, LX, LA, K


def main(name: str = "qp_weights.npz"):
    with np.load(HERE / "qp_terrain.npz") as z:
        batch = {k: z[k] for k in KEYS}
    out = dict(batch)
    for tag, wt in weight_sets().items():
        W, LX, LA, K = certify(batch, wt)
        out.update({f"Q_{tag}": wt["Q"].astype(np.float32), f"R_{tag}": wt["R"].astype(np.float32),
                    f"w_{tag}": W, f"lam_x_{tag}": LX, f"lam_a_{tag}": LA, f"kkt_{tag}": K})
        print(f"set {tag}: max KKT {K.max():.2e}")
    np.savez_compressed(HERE / name, **out)
    print(name, (HERE / name).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
