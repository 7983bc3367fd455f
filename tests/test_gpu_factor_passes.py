"""The passes around the factorization's and the condensation's MFMAs -- the unit-diagonal scaling
and un-scaling of ldl_tiles, the sweep's panel publish and operand build (sweep_publish,
sweep_operands, pivot_block), the closed form's V build, operand cache and step sums
(condense_tiles_nil, step_sums) and the same helpers in the team factor -- at the smallest shapes
where their lane, tile and pivot-step edges lie.

Free-force counts n (multiples of 3; two instances each, built as test_gpu_heavy_paths.edge_batch
builds its own), at horizon N = 16:
  3, 6            one partial 4-pivot step; a second step of 2 pivots
  12, 15, 18      a full block row; a tile whose last step has 3 pivots and one padding row; the
                  first step of block 1 with subs == 1 (the pipelined loop body is skipped and the
                  block-opening path runs with has_next false)
  48, 51          has_next false exactly on a tile edge, and one step past it
  63, 66          the un-scaling pass's second trip of 64 lanes
  96 / 99, 126 / 129, 141 / 144 / 147, 159 / 162, 189 / 192
                  each bin's last tile and the next bin's first row; odd and even TT - KMIN
and n = 3, 6, 9, 12 at horizons N = 1 and N = 5: the step sums at k = 0 and at k = N - 1.  A subset
(DAMPED) is solved again with the attitude-damped step matrix of test_gpu_admm_passes.damped_batch,
which is not I + N with N^2 = 0: the general condensations, whose condense_finish and sweep are
the same code.

Every optimum is certified in tests/golden/qp_factor_passes.npz (tests/golden/
make_factor_passes.py: oracle/tight_solver.py, KKT residuals below 1e-8 on every instance, with
the digests of the inputs).  Each batch is solved by the wave kernels (team mode off) and by the
team kernel (team mode forced).

Tolerance (as tests/test_gpu_heavy_paths.py): contact forces within 1e-4 relative of the
certified float64 optimum at status 1; a batch may hold at most one status 2, within 1e-3; the
states within 1e-4 of the float64 rollout of the forces.
"""
import numpy as np
import pytest

from parity_util import (load_fixture, rel_err_U, split_w, rollout64, assert_verified,
                         input_digest)
from test_gpu_heavy_paths import edge_batch, _count

pytestmark = pytest.mark.gpu
TOL_U = 1e-4
KEYS = ("Ad", "Bd", "gd", "x0", "xref", "contact")
MODES = {"wave": 0, "team": 1 << 40}
PER_N = 2
# batch name -> (horizon, free-force counts, seed of the draw)
BATCHES = {
    "small": (16, (3, 6, 12, 15, 18, 48, 51, 63, 66), 53),
    "bins": (16, (96, 99, 126, 129, 141, 144, 147, 159, 162, 189, 192), 59),
    "n1": (1, (3, 6, 9, 12), 61),
    "n5": (5, (3, 6, 9, 12), 67),
}
# (batch, instance) solved again with the damped step matrix: n = 6, 18, 51, 66 and
# n = 99, 129, 147, 162, 192
DAMPED = (("small", 2), ("small", 8), ("small", 12), ("small", 16),
          ("bins", 2), ("bins", 6), ("bins", 12), ("bins", 16), ("bins", 20))
DAMPED_N = (6, 18, 51, 66, 99, 129, 147, 162, 192)


def batch(name):
    N, targets, seed = BATCHES[name]
    return edge_batch(N=N, per_n=PER_N, targets=targets, seed=seed)


def damped_batch():
    """DAMPED with the step matrix of test_gpu_admm_passes.damped_batch."""
    bs = {name: batch(name) for name in ("small", "bins")}
    b = {k: np.stack([bs[name][k][i] for name, i in DAMPED]).astype(np.float64) for k in KEYS}
    for r in range(3, 6):
        b["Ad"][:, r, r] = 0.999
    return b


@pytest.fixture(scope="module")
def fx():
    f = load_fixture("qp_factor_passes.npz")
    for v in f.values():
        v.setflags(write=False)
    return f


def _plan(mode, N=16):
    from cmpc import Plan, SolverParams
    p = Plan(SolverParams(N=N, max_batch=64))
    p.set_team(MODES[mode])
    return p


def _check(b, w, st, ref, N):
    ok = assert_verified(st)
    err = rel_err_U(w, ref, N=N)
    print("status", st.tolist())
    print("rel err", err.tolist())
    for i in range(len(err)):
        assert err[i] <= (TOL_U if ok[i] else 1e-3), (i, int(st[i]), err[i])
    Xg, Ug = split_w(w.astype(np.float64), N)
    assert np.max(np.abs(Xg - rollout64(b, Ug))) < 1e-4


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(BATCHES))
def test_count_edges(fx, name, mode):
    from cmpc import solve_batch
    N, targets, _ = BATCHES[name]
    b = batch(name)
    assert input_digest(b, np.arange(len(b["Ad"]))) == str(fx[f"digest_{name}"]), "generator drifted"
    assert (3 * _count(b["contact"])).tolist() == [n for n in targets for _ in range(PER_N)]
    w, st, it = solve_batch(b, plan=_plan(mode, N))
    assert w.shape == (len(b["Ad"]), 24 * N)
    print("iters", it.tolist())
    _check(b, w, st, fx[f"w_{name}"], N)


@pytest.mark.parametrize("mode", list(MODES))
def test_damped_step_matrix(fx, mode):
    from cmpc import solve_batch
    b = damped_batch()
    assert input_digest(b, np.arange(len(DAMPED))) == str(fx["digest_damped"]), "generator drifted"
    assert (3 * _count(b["contact"])).tolist() == list(DAMPED_N)
    Nm = b["Ad"][0].astype(np.float32) - np.eye(12, dtype=np.float32)
    assert np.any(Nm @ Nm != 0)
    w, st, it = solve_batch(b, plan=_plan(mode))
    print("iters", it.tolist())
    _check(b, w, st, fx["w_damped"], 16)
