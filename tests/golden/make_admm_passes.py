"""Certified optima of tests/test_gpu_admm_passes.py's batches -> qp_admm_passes.npz (CPU, a minute
or two): oracle/tight_solver.py on every instance of the N = 16, 5 and 1 batches and of the damped
subset, KKT residuals below 1e-8 (make_heavy_edges.optima asserts it per instance), with the
sha256 digest of each batch's inputs (parity_util.input_digest) so that the test notices a drifted
generator.
    python tests/golden/make_admm_passes.py
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
import test_gpu_admm_passes as T                   # noqa: E402


if __name__ == "__main__":
    out = {}
    for N in T.STEPS:
        b = T.batch(N)
        out[f"w{N}"] = optima(b)
        out[f"digest{N}"] = input_digest(b, np.arange(len(b["Ad"])))
        out[f"n{N}"] = 3 * T._count(b["contact"])
        print("N", N, "n", out[f"n{N}"].tolist())
    b = T.damped_batch()
    out["w_damped"] = optima(b)
    out["digest_damped"] = input_digest(b, np.arange(len(b["Ad"])))
    np.savez_compressed(REPO / "tests" / "golden" / "qp_admm_passes.npz", **out)
    print("wrote qp_admm_passes.npz")
