"""Certified optima of tests/test_gpu_heavy_paths.py's batches -> qp_heavy_edges.npz (CPU, about
a minute): oracle/tight_solver.py on every instance, KKT residuals below 1e-8, with the sha256
digest of the inputs (parity_util.input_digest) so that the test notices a drifted generator.
    python tests/golden/make_heavy_edges.py"""
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(REPO), str(REPO / "convex-mpc-unitree-go2_amd"), str(REPO / "tests")]

from oracle import mpc_qp, tight_solver            # noqa: E402
from parity_util import input_digest               # noqa: E402
import test_gpu_heavy_paths as T                   # noqa: E402


def optima(b):
    out = []
    for i in range(len(b["Ad"])):
        qp = mpc_qp.build_qp(b["Ad"][i], b["Bd"][i], b["gd"][i], b["x0"][i], b["xref"][i].T,
                             b["contact"][i])
        r = tight_solver.solve(qp)
        assert max(r["kkt"].values()) < 1e-8, (i, r["kkt"])
        out.append(r["w"])
    return np.stack(out)


if __name__ == "__main__":
    b16, b8 = T.edge_batch(), T.edge_batch(**T.SHORT)
    np.savez_compressed(REPO / "tests" / "golden" / "qp_heavy_edges.npz",
                        w=optima(b16), digest=input_digest(b16, np.arange(len(b16["Ad"]))),
                        n=3 * T._count(b16["contact"]),
                        w8=optima(b8), digest8=input_digest(b8, np.arange(len(b8["Ad"]))),
                        n8=3 * T._count(b8["contact"]))
    print("wrote qp_heavy_edges.npz", len(b16["Ad"]), len(b8["Ad"]))
