"""Certified optima and multipliers of tests/test_gpu_instance_passes.py's batches ->
qp_instance_passes.npz (CPU, a minute or two): oracle/tight_solver.py on every instance of the
count batches, the batches with empty steps and the damped subset, KKT residuals below 1e-8 on every
instance (asserted as make_heavy_edges.optima asserts them), with the sha256 digest of each batch's
inputs (parity_util.input_digest) so that the test notices a drifted generator.
    python tests/golden/make_instance_passes.py
The linear algebra runs on one thread, as in make_factor_passes.py: the run is then the same
everywhere."""
import os
import sys
from pathlib import Path

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"

import numpy as np                                 # noqa: E402

REPO = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(REPO), str(REPO / "convex-mpc-unitree-go2_amd"), str(REPO / "tests"),
                str(REPO / "tests" / "golden")]

from oracle import mpc_qp, tight_solver            # noqa: E402
from parity_util import input_digest               # noqa: E402
from make_heavy_edges import optima                # noqa: E402
import test_gpu_instance_passes as T               # noqa: E402


def multipliers(b, w):
    """The certified multipliers of every instance; the optimum must be make_heavy_edges.optima's
    (the same solver on the same problem)."""
    lx, la = [], []
    for i in range(len(b["Ad"])):
        qp = mpc_qp.build_qp(b["Ad"][i], b["Bd"][i], b["gd"][i], b["x0"][i], b["xref"][i].T,
                             b["contact"][i])
        r = tight_solver.solve(qp)
        assert max(r["kkt"].values()) < 1e-8, (i, r["kkt"])
        assert np.array_equal(r["w"], w[i]), i
        lx.append(r["lam_x"])
        la.append(r["lam_a"])
    return np.stack(lx), np.stack(la)


def certify(out, name, b):
    w = optima(b)
    out[f"w_{name}"] = w
    out[f"lam_x_{name}"], out[f"lam_a_{name}"] = multipliers(b, w)
    out[f"digest_{name}"] = input_digest(b, np.arange(len(b["Ad"])))
    out[f"n_{name}"] = 3 * T._count(b["contact"])
    print(name, "n", out[f"n_{name}"].tolist(), flush=True)


if __name__ == "__main__":
    out = {}
    for name in T.BATCHES:
        certify(out, name, T.batch(name))
    certify(out, "damped", T.damped_batch())
    np.savez_compressed(REPO / "tests" / "golden" / "qp_instance_passes.npz", **out)
    print("wrote qp_instance_passes.npz")
