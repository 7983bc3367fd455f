"""Certified optima of tests/test_gpu_factor_passes.py's batches -> qp_factor_passes.npz (CPU, a
minute or two): oracle/tight_solver.py on every instance of the four count batches and of the
damped subset, KKT residuals below 1e-8 (make_heavy_edges.optima asserts it per instance), with the
sha256 digest of each batch's inputs (parity_util.input_digest) so that the test notices a drifted
generator.
    python tests/golden/make_factor_passes.py
The linear algebra runs on one thread, as in make_tile_edges.py: the run is then the same
everywhere."""
import os
import sys
from pathlib import Path

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"

import numpy as np                                 # noqa: E402

REPO = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(REPO), str(REPO / "convex-mpc-unitree-go2_amd"), str(REPO / "tests")]

from parity_util import input_digest               # noqa: E402
from make_heavy_edges import optima                # noqa: E402
import test_gpu_factor_passes as T                 # noqa: E402


if __name__ == "__main__":
    out = {}
    for name in T.BATCHES:
        b = T.batch(name)
        out[f"w_{name}"] = optima(b)
        out[f"digest_{name}"] = input_digest(b, np.arange(len(b["Ad"])))
        out[f"n_{name}"] = 3 * T._count(b["contact"])
        print(name, "n", out[f"n_{name}"].tolist())
    b = T.damped_batch()
    out["w_damped"] = optima(b)
    out["digest_damped"] = input_digest(b, np.arange(len(b["Ad"])))
    out["n_damped"] = 3 * T._count(b["contact"])
    print("damped n", out["n_damped"].tolist())
    np.savez_compressed(REPO / "tests" / "golden" / "qp_factor_passes.npz", **out)
    print("wrote qp_factor_passes.npz")
