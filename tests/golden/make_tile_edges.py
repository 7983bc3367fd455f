"""Certified optima of tests/test_gpu_fixup_passes.py's batch -> qp_tile_edges.npz (CPU, about a
minute): oracle/tight_solver.py on every instance, KKT residuals below 1e-8, with the sha256
digest of the inputs (parity_util.input_digest) so that the test notices a drifted generator.
    python tests/golden/make_tile_edges.py
The linear algebra runs on one thread: the interior-point iteration of one n = 3 instance is
sensitive to the BLAS blocking (it misses the 1e-8 certificate at eight threads), and with one
thread the run is the same everywhere."""
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
import test_gpu_fixup_passes as T                  # noqa: E402


if __name__ == "__main__":
    b = T.tile_edge_batch()
    np.savez_compressed(REPO / "tests" / "golden" / "qp_tile_edges.npz",
                        w=optima(b), digest=input_digest(b, np.arange(len(b["Ad"]))),
                        n=3 * T._count(b["contact"]))
    print("wrote qp_tile_edges.npz", len(b["Ad"]))
