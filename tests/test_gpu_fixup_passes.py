"""The fix-up passes around the condensation's and the factorization's MFMA cores -- the diagonal
mirror, + diag(Rt) + shift with the identity on padding, the unit-diagonal scaling and its
undoing -- at the tile and padding edges, where alone they can go wrong.

Free-force counts n (3 per stance (step, leg) pair), two instances each: 3, 15, 18 and 48 (one
tile; a second tile with two real rows; a full third tile), 93 and 96 (NC 96: one padding row
group, none), 99, 111 and 114 (NC 128: three real rows in the seventh tile, one real row short of
a full one, two rows into the eighth), 126 and 129 (the last tile of NC 128; one real row in the
ninth of NC 144), 144 and 147, 159 and 162 (the edges of the one-wave bins), 192 (no padding at
all) and 0 (all swing).  The batch is built as tests/test_gpu_heavy_paths.py::edge_batch builds
its own and certified in tests/golden/qp_tile_edges.npz (tests/golden/make_tile_edges.py:
oracle/tight_solver.py, KKT residuals below 1e-8, with the digest of the inputs).  It is solved
by the wave kernels (team mode off) and by the team kernel (team mode forced); the polish basis
hands the same passes arbitrary nact on the way.

Tolerance (as tests/test_gpu_heavy_paths.py): contact forces within 1e-4 relative of the
certified float64 optimum at status 1; a small batch may hold at most one status 2, within 1e-3.
"""
import numpy as np
import pytest

from parity_util import (load_fixture, rel_err_U, split_w, rollout64, assert_verified,
                         input_digest)
from test_gpu_heavy_paths import edge_batch, _count

pytestmark = pytest.mark.gpu
TOL_U = 1e-4
KEYS = ("Ad", "Bd", "gd", "x0", "xref", "contact")
TILE_N = (3, 15, 18, 48, 93, 96, 99, 111, 114, 126, 129, 144, 147, 159, 162, 192, 0)
PER_N = 2
MODES = {"wave": 0, "team": 1 << 40}


def tile_edge_batch():
    return edge_batch(per_n=PER_N, targets=TILE_N, seed=37)


@pytest.fixture(scope="module")
def edges():
    """The batch and its certified optima."""
    fx = load_fixture("qp_tile_edges.npz")
    b = tile_edge_batch()
    assert (3 * _count(b["contact"])).tolist() == [n for n in TILE_N for _ in range(PER_N)]
    assert input_digest(b, np.arange(len(b["Ad"]))) == str(fx["digest"]), "generator drifted"
    ref = fx["w"]
    ref.setflags(write=False)
    return b, ref


def _plan(mode):
    from cmpc import Plan, SolverParams
    p = Plan(SolverParams(max_batch=64))
    p.set_team(MODES[mode])
    return p


@pytest.fixture(scope="module")
def solved(edges):
    """The batch solved in both modes, once."""
    from cmpc import solve_batch
    b, _ = edges
    return {mode: solve_batch(b, plan=_plan(mode)) for mode in MODES}


@pytest.mark.parametrize("mode", list(MODES))
def test_tile_edge_parity(edges, solved, mode):
    b, ref = edges
    w, st, it = solved[mode]
    ok = assert_verified(st)
    err = rel_err_U(w, ref)
    print("status", st.tolist())
    print("rel err", err.tolist())
    for i in range(len(err)):
        assert err[i] <= (TOL_U if ok[i] else 1e-3), (i, int(st[i]), err[i])
    Xg, Ug = split_w(w.astype(np.float64))
    swing = 3 * _count(b["contact"]) == 0
    assert np.all(Ug[swing] == 0)
    assert np.max(np.abs(Xg - rollout64(b, Ug))) < 1e-4


@pytest.mark.parametrize("mode", list(MODES))
def test_tile_edge_reversed_order_bitwise(edges, solved, mode):
    """The same batch in reversed instance order: every instance lands on another wave (or
    team), after other instances; its outputs are bitwise the same."""
    from cmpc import solve_batch
    b, _ = edges
    w0, s0, i0 = solved[mode]
    w1, s1, i1 = solve_batch({k: b[k][::-1].copy() for k in KEYS}, plan=_plan(mode))
    w1, s1, i1 = w1[::-1], s1[::-1], i1[::-1]
    same = np.all(w0.view(np.uint32) == w1.view(np.uint32), axis=1) & (s0 == s1) & (i0 == i1)
    assert same.all(), np.flatnonzero(~same).tolist()


def test_tile_edge_general_step_matrix(edges):
    """A step matrix that is not I + N, N^2 = 0 (the attitude-damped Ad of
    test_gpu_heavy_paths.py::test_general_step_matrix_edges) on n = 111 and n = 129.  Team mode
    off, at a batch this small (latency mode): n = 111 takes the block-row condensation (diagonal
    mirror, then the finish), n = 129 the forward one (the finish alone); team mode forced: the
    team factor's general branch and its scaling.  Certified on the CPU as there
    (oracle/active_set.py, seeded by the GPU's answer), with its rule: at most one status 2,
    within 1e-3."""
    from cmpc import solve_batch
    from oracle import active_set, mpc_qp
    b0, _ = edges
    pick = [TILE_N.index(n) * PER_N for n in (111, 129)]
    b = {k: b0[k][pick].astype(np.float64) for k in KEYS}
    for r in range(3, 6):
        b["Ad"][:, r, r] = 0.999
    Nm = b["Ad"][0].astype(np.float32) - np.eye(12, dtype=np.float32)
    assert np.any(Nm @ Nm != 0)
    got = {mode: solve_batch(b, plan=_plan(mode)) for mode in MODES}
    cert = []
    for i in range(len(pick)):
        qp = mpc_qp.build_qp(b["Ad"][i], b["Bd"][i], b["gd"][i], b["x0"][i], b["xref"][i].T,
                             b["contact"][i])
        r = active_set.certified_optimum(qp, got["wave"][0][i].astype(np.float64))
        assert max(r["kkt"].values()) <= active_set.CERT_TOL, i
        cert.append(r["w"])
    for mode, (w, st, it) in got.items():
        print(mode, "status", st.tolist(), "iters", it.tolist())
        ok = assert_verified(st)
        err = rel_err_U(w, np.stack(cert))
        print(mode, "rel err", err.tolist())
        for i in range(len(pick)):
            assert err[i] <= (TOL_U if ok[i] else 1e-3), (mode, i, int(st[i]), err[i])
