"""The passes that run every ADMM iteration -- the LDL' solve (ldl_apply), the gradient's per-step
sum and its closing B~' lambda + R~ v loop, and the iteration's own bookkeeping (the rho
adaptation and polish-trigger periods, the last iteration) -- at the smallest shapes where their
lane, tile and per-step edges lie.

Per-step parameter counts (step_batch, one contact table per instance, a letter per step: f all
four legs = 12 params, e no stance leg, 1 one leg, p the drawn table's own column, which holds at
least one stance leg): an empty step between two that have some (off[c] == off[c + 1]), a full
step, an empty first and an empty last step, a run of empty steps, at horizons N = 16, 5 and 1.
Free-force counts n (COUNT_N, two instances each, built as test_gpu_heavy_paths.edge_batch builds
its own): 63 and 66 (the closing loop's second trip of 64 lanes), 96 and 99 (NC 96 full; the first
NC 128 instance), 126 and 129 (the last tile of NC 128; the first row of the ninth tile of NC 144).
The remaining tile edges come from tests/golden/qp_tile_edges.npz, read only.  A subset is solved
again with an attitude-damped step matrix, which is not I + N with N^2 = 0: the gradient's general
scans and the forward condensation.

Every optimum is certified in tests/golden/qp_admm_passes.npz (tests/golden/make_admm_passes.py:
oracle/tight_solver.py, KKT residuals below 1e-8 on every instance, with the digests of the
inputs).  Each batch is solved by the wave kernels (team mode off) and by the team kernel (team
mode forced).

Tolerance (as tests/test_gpu_heavy_paths.py): contact forces within 1e-4 relative of the
certified float64 optimum at status 1; a batch may hold at most one status 2, within 1e-3.
"""
import numpy as np
import pytest

from parity_util import (load_fixture, rel_err_U, split_w, rollout64, assert_verified,
                         input_digest)
from test_gpu_heavy_paths import edge_batch, _count
from test_gpu_fixup_passes import tile_edge_batch

pytestmark = pytest.mark.gpu
TOL_U = 1e-4
KEYS = ("Ad", "Bd", "gd", "x0", "xref", "contact")
MODES = {"wave": 0, "team": 1 << 40}
COUNT_N = (63, 66, 96, 99, 126, 129)
PER_N = 2
STEPS = {
    16: ("ppepfppppppppppp", "e" + "p" * 14 + "e", "e" + "p" * 6 + "ef" + "p" * 6 + "e",
         "f" + "e" * 14 + "f"),
    5: ("fepfe", "epppp", "fffff", "ppepp", "1e1e1"),
    1: ("f", "p", "1", "e"),
}
# instances of batch(16) solved again with the damped step matrix: the empty step and the full
# one, the run of empty steps, and n = 63, 96, 129
DAMPED = (0, 3, 4, 8, 14)


def step_batch(N):
    """One instance per entry of STEPS[N]: a config-2 draw at horizon N under that contact table
    (a leg turned to stance has a zero lever in Bd, as in edge_batch)."""
    from cmpc import synth
    pool = synth.make_batch(len(STEPS[N]), seed=43 + N, mixed=True, N=N)
    ct = pool["contact"].copy()                      # (B, 4, N)
    for i, spec in enumerate(STEPS[N]):
        assert len(spec) == N
        for k, ch in enumerate(spec):
            if ch != "p":
                ct[i, :, k] = {"f": (1, 1, 1, 1), "e": (0, 0, 0, 0), "1": (1, 0, 0, 0)}[ch]
            else:
                assert ct[i, :, k].any()
    out = {k: pool[k] for k in KEYS}
    out["contact"] = ct
    return out


def batch(N):
    """N = 16: the step tables, then the counts of COUNT_N; N = 5, 1: the step tables."""
    b = step_batch(N)
    if N == 16:
        e = edge_batch(per_n=PER_N, targets=COUNT_N, seed=41)
        b = {k: np.concatenate([b[k], e[k]]) for k in KEYS}
    return b


def damped_batch():
    b0 = batch(16)
    b = {k: b0[k][list(DAMPED)].astype(np.float64) for k in KEYS}
    for r in range(3, 6):
        b["Ad"][:, r, r] = 0.999
    return b


@pytest.fixture(scope="module")
def fx():
    f = load_fixture("qp_admm_passes.npz")
    for v in f.values():
        v.setflags(write=False)
    return f


def _plan(mode, N=16, **params):
    from cmpc import Plan, SolverParams
    p = Plan(SolverParams(N=N, max_batch=64, **params))
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
    swing = _count(b["contact"]) == 0
    assert np.all(Ug[swing] == 0)
    assert np.max(np.abs(Xg - rollout64(b, Ug))) < 1e-4


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("N", list(STEPS))
def test_step_and_count_edges(fx, N, mode):
    from cmpc import solve_batch
    b = batch(N)
    assert input_digest(b, np.arange(len(b["Ad"]))) == str(fx[f"digest{N}"]), "generator drifted"
    if N == 16:
        assert (3 * _count(b["contact"]))[len(STEPS[16]):].tolist() == \
            [n for n in COUNT_N for _ in range(PER_N)]
        per_step = b["contact"][0].sum(0)
        assert per_step[2] == 0 and per_step[1] > 0 and per_step[3] > 0 and per_step[4] == 4
    w, st, it = solve_batch(b, plan=_plan(mode, N))
    assert w.shape == (len(b["Ad"]), 24 * N)
    _check(b, w, st, fx[f"w{N}"], N)


@pytest.mark.parametrize("mode", list(MODES))
def test_damped_step_matrix(fx, mode):
    """The step matrix of test_gpu_heavy_paths.py::test_general_step_matrix_edges on DAMPED."""
    from cmpc import solve_batch
    b = damped_batch()
    assert input_digest(b, np.arange(len(DAMPED))) == str(fx["digest_damped"]), "generator drifted"
    Nm = b["Ad"][0].astype(np.float32) - np.eye(12, dtype=np.float32)
    assert np.any(Nm @ Nm != 0)
    w, st, it = solve_batch(b, plan=_plan(mode))
    print("iters", it.tolist())
    _check(b, w, st, fx["w_damped"], 16)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("params", [dict(adaptive_rho_interval=3), dict(check_termination=4)],
                         ids=["adapt3", "check4"])
def test_short_periods(fx, params, mode):
    """rho adapts every third iteration (the period wraps several times before the first polish
    session), or a polish session may start only at every fourth: the same optima, on this file's
    N = 16 batch and on the tile-edge batch."""
    from cmpc import solve_batch
    b = batch(16)
    w, st, it = solve_batch(b, plan=_plan(mode, **params))
    print("iters", it.tolist())
    _check(b, w, st, fx["w16"], 16)
    te = load_fixture("qp_tile_edges.npz")
    b = tile_edge_batch()
    assert input_digest(b, np.arange(len(b["Ad"]))) == str(te["digest"]), "generator drifted"
    w, st, it = solve_batch(b, plan=_plan(mode, **params))
    print("iters", it.tolist())
    _check(b, w, st, te["w"], 16)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("params", [dict(max_iter=3), dict(max_iter=4, adaptive_rho_interval=2)],
                         ids=["iter3", "iter4_adapt2"])
def test_last_iteration(params, mode):
    """ADMM stopped after a few iterations, before any polish session can start (the face set
    must first stay unchanged for polish_stable = 3 iterations, and the last iteration starts
    none); in the second case the last iteration is also one at which rho would adapt.  Every
    instance (each has stance legs) returns status 2 or -2 at iters == max_iter, finite, with
    states that are the rollout of its forces.  Which of the two statuses is right, and the
    iterates themselves, are checked against the float64 reference in
    tests/test_gpu_admm_iterates.py (test_exit_status, test_iterates_default)."""
    from cmpc import solve_batch
    b = batch(16)
    w, st, it = solve_batch(b, plan=_plan(mode, **params))
    print("status", st.tolist(), "iters", it.tolist())
    assert np.all((st == 2) | (st == -2)), st
    assert np.all(it == params["max_iter"]), it
    assert np.all(np.isfinite(w))
    Xg, Ug = split_w(w.astype(np.float64))
    assert np.max(np.abs(Xg - rollout64(b, Ug))) < 1e-4
