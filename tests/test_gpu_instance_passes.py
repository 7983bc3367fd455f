"""What an instance runs once, or once per polish session -- stage_instance (the d_k loop, the
nilpotent test), build_admm_basis, starting_point, polish_setup (at a session's opening, on the ADMM
basis, and inside a session, on a reduced one; its d~ loop, which finds the triples that lock fz
from the wave's stance and face masks) and the writers of w, y and lam -- at the smallest shapes
where their lane, trip and layout edges lie.

Stance triples t (free forces n = 3 t; two instances each, built as
test_gpu_heavy_paths.edge_batch builds its own), at horizon N = 16:
  0, 1            all swing (n = 0: status 1, zero forces, X the rollout) and a single triple
  21, 22          n = 63 / 66: the 64-lane trip edge of the fill loops
  32 / 33, 42 / 43, 48 / 49, 53 / 54
                  n = 96 / 99, 126 / 129, 144 / 147, 159 / 162: the bin edges
  63, 64          n = 189 / 192: every lane owns a triple
and at N = 5 (t = 0, 1, 10, 19, 20) and N = 1 (t = 0, 1, 3, 4): the 12 N loops make one trip and
a partial one (N = 16: three), lanes >= 4 N own no (step, leg), off[] has N + 1 entries.  The "gaps"
batches are test_gpu_admm_passes.step_batch's tables with a step that has no stance foot at the
start, in the middle and at the end (off[k] == off[k + 1]) at N = 16 and N = 5.  A subset (DAMPED)
is solved again with the attitude-damped step matrix of test_gpu_admm_passes.damped_batch, which is
not I + N with N^2 = 0 (asserted in fp32).

Every optimum and its multipliers are certified in tests/golden/qp_instance_passes.npz
(tests/golden/make_instance_passes.py: oracle/tight_solver.py, KKT residuals below 1e-8 on every
instance, with the digests of the inputs).  Each batch is solved by the wave kernels (team mode
off) and by the team kernel (team mode forced), with lam_out, and once more with y_out.

Starts (test_starts): cold, w_init alone, w_init + y_init, w_init + lam_init, and non-finite warm
data, which falls back to a cold start; a warm session opens with polish_setup right after the
staging, before any ADMM iteration.  Each is compared with the certified optimum at the same
tolerance.

Per-instance mu / fz_min and Q / R (test_terrain_and_weights): tests/golden/qp_terrain.npz and
qp_weights.npz, read only, with one invalid row each (status -10, zero forces, X the rollout).

Sessions (test_sessions): tests/golden/qp_hard.npz and qp_cfg2.npz, read only.  Traced in wave
mode with a -DCMPC_TRACE_IDS build of this library (the build tools/trace_batch.py loads):
  qp_hard[2], qp_hard[3]   the first polish session fails after repairs that drop faces (each a
                           refactor_faces: polish_setup on a reduced basis, from global memory),
                           session_failed rebuilds the ADMM basis from global memory, the second
                           session (polish_setup on that basis) fails too and restores the parked
                           inverse; solved after 139 and 93 iterations
  qp_hard[0]               three faces added by downdates, no refactorization inside the session
  qp_hard[1]               four faces added by a downdate, then a repair that drops faces
  qp_cfg2[23], qp_cfg2[24] a downdated refinement stalls: kRefactorSameSet, polish_setup from the
                           candidate forces in s.dl
  qp_cfg2[0], qp_cfg2[39]  a repair that drops faces in the first session

Tolerance (as tests/test_gpu_factor_passes.py): contact forces within 1e-4 relative of the
certified float64 optimum at status 1; a batch may hold at most one status 2, within 1e-3
(parity_util.assert_verified); the states within 1e-4 of the float64 rollout of the forces.
Multipliers as tests/test_gpu_duals.py: max |lam - lam*| <= 1e-4 max |lam*| per instance at status
1; y, the force dual, against the same certified multipliers through the relation starting_point
documents (y = F' lam_fric + lam_x[u] on stance legs, zero on swing legs).  y is a combination of
the multipliers and, like them, a difference of terms of the multipliers' size (-grad f(u) in
fp32), so it is held to their bar on their scale: max |y - y*| <= 1e-4 max |lam*| per instance.
"""
import numpy as np
import pytest

from parity_util import (load_fixture, fixture_batch, rel_err_U, split_w, rollout64,
                         assert_verified, input_digest)
from test_gpu_heavy_paths import edge_batch, _count
from test_gpu_admm_passes import step_batch

pytestmark = pytest.mark.gpu
TOL = 1e-4
KEYS = ("Ad", "Bd", "gd", "x0", "xref", "contact")
MODES = {"wave": 0, "team": 1 << 40}
PER_N = 2
# batch name -> (horizon, stance triples, seed of the draw)
COUNTS = {
    "light": (16, (0, 1, 21, 22, 32, 33), 71),
    "heavy": (16, (42, 43, 48, 49, 53, 54, 63, 64), 73),
    "n5": (5, (0, 1, 10, 19, 20), 79),
    "n1": (1, (0, 1, 3, 4), 83),
}
# batch name -> (horizon, rows of step_batch(horizon)): "e" + "p" * 14 + "e" and
# "e" + "p" * 6 + "ef" + "p" * 6 + "e"; "fepfe" and "epppp"
GAPS = {"gaps16": (16, (1, 2)), "gaps5": (5, (0, 1))}
BATCHES = tuple(COUNTS) + tuple(GAPS)
# (batch, instance) solved again with the damped step matrix: t = 1, 22, 33 and 43, 49, 54, 64,
# and the N = 16 table with empty steps at the start, in the middle and at the end
DAMPED = (("light", 2), ("light", 6), ("light", 10), ("heavy", 2), ("heavy", 6), ("heavy", 10),
          ("heavy", 14), ("gaps16", 1))
DAMPED_T = (1, 22, 33, 43, 49, 54, 64)


def horizon(name):
    return COUNTS[name][0] if name in COUNTS else GAPS[name][0]


def batch(name):
    if name in COUNTS:
        N, tris, seed = COUNTS[name]
        return edge_batch(N=N, per_n=PER_N, targets=tuple(3 * t for t in tris), seed=seed)
    N, rows = GAPS[name]
    b = step_batch(N)
    return {k: b[k][list(rows)] for k in KEYS}


def damped_batch():
    bs = {name: batch(name) for name in ("light", "heavy", "gaps16")}
    b = {k: np.stack([bs[name][k][i] for name, i in DAMPED]).astype(np.float64) for k in KEYS}
    for r in range(3, 6):
        b["Ad"][:, r, r] = 0.999
    return b


@pytest.fixture(scope="module")
def fx():
    f = load_fixture("qp_instance_passes.npz")
    for v in f.values():
        v.setflags(write=False)
    return f


def _plan(mode, N=16):
    from cmpc import Plan, SolverParams
    p = Plan(SolverParams(N=N, max_batch=64))
    p.set_team(MODES[mode])
    return p


def _solve(plan, b, **kw):
    """Numpy batch in, numpy results out: (w, status, iters[, dual])."""
    import torch
    from cmpc import to_device_batch
    d = to_device_batch({k: b[k] for k in KEYS}, plan.device)
    t = {k: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32)).to(plan.device)
         if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    r = plan.solve(*(d[k] for k in KEYS), **t)
    torch.cuda.synchronize(plan.device)
    return tuple(x.cpu().numpy() for x in r)


def _check(b, w, st, ref, N, bad=()):
    """Forces, statuses and states of a solved batch; `bad` lists the invalid rows (status -10)."""
    good = np.array([i not in bad for i in range(len(st))])
    assert np.all(st[~good] == -10), st
    ok = np.zeros(len(st), dtype=bool)
    ok[good] = assert_verified(st[good])
    err = rel_err_U(w, ref, N=N)
    print("status", st.tolist())
    print("rel err", err.tolist())
    for i in np.flatnonzero(good):
        assert err[i] <= (TOL if ok[i] else 1e-3), (i, int(st[i]), err[i])
    Xg, Ug = split_w(w.astype(np.float64), N)
    zero = (_count(b["contact"]) == 0) | ~good
    assert np.all(Ug[zero] == 0)
    assert np.max(np.abs(Xg - rollout64(b, Ug))) < 1e-4
    return ok


def _lam_err(lam, lam_x, lam_a):
    ref = np.concatenate([lam_x, lam_a], axis=1)
    scale = np.maximum(np.max(np.abs(ref), axis=1), 1e-9)
    err = np.max(np.abs(lam.astype(np.float64) - ref), axis=1) / scale
    print("lam err", err.tolist())
    return err


def y_of(lam_x, lam_a, contact, N, mu):
    """The force dual of the certified multipliers, in the force layout [k][leg][axis]:
    y = F' lam_fric + lam_x[u] on stance legs (rows fx - mu fz, -fx - mu fz, fy - mu fz,
    -fy - mu fz), zero on swing legs."""
    B = len(lam_x)
    lx = lam_x[:, 12 * N:].reshape(B, N, 4, 3)
    lf = lam_a[:, 12 * N:].reshape(B, N, 4, 4)
    y = np.stack([lf[..., 0] - lf[..., 1] + lx[..., 0], lf[..., 2] - lf[..., 3] + lx[..., 1],
                  -mu * lf.sum(-1) + lx[..., 2]], axis=-1)
    y *= (contact.transpose(0, 2, 1) != 0)[..., None]
    return y.reshape(B, 12 * N)


def _y_err(y, yref, lam_x, lam_a):
    scale = np.maximum(np.max(np.abs(np.concatenate([lam_x, lam_a], axis=1)), axis=1), 1e-9)
    err = np.max(np.abs(y.astype(np.float64) - yref), axis=1) / scale
    print("y err", err.tolist())
    return err


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", BATCHES)
def test_count_and_step_edges(fx, name, mode):
    N = horizon(name)
    b = batch(name)
    B = len(b["Ad"])
    assert input_digest(b, np.arange(B)) == str(fx[f"digest_{name}"]), "generator drifted"
    if name in COUNTS:
        assert _count(b["contact"]).tolist() == [t for t in COUNTS[name][1] for _ in range(PER_N)]
    else:
        per_step = (b["contact"] != 0).sum(1)            # (B, N)
        assert np.all((per_step[:, 0] == 0) | (per_step[:, -1] == 0))
        assert np.all((per_step == 0).any(1))
    plan = _plan(mode, N)
    w, st, it, lam = _solve(plan, b, lam_out=True)
    assert w.shape == (B, 24 * N) and lam.shape == (B, 52 * N)
    print("iters", it.tolist())
    ok = _check(b, w, st, fx[f"w_{name}"], N)
    swing = _count(b["contact"]) == 0
    assert np.all(st[swing] == 1)
    err = _lam_err(lam, fx[f"lam_x_{name}"], fx[f"lam_a_{name}"])
    assert np.all(err[ok] <= TOL), err
    w2, st2, it2, y = _solve(plan, b, y_out=True)
    assert np.array_equal(w2.view(np.uint32), w.view(np.uint32)) and np.array_equal(st2, st)
    lx, la = fx[f"lam_x_{name}"], fx[f"lam_a_{name}"]
    yerr = _y_err(y, y_of(lx, la, b["contact"], N, plan.params.mu), lx, la)
    assert np.all(yerr[ok & ~swing] <= TOL), yerr
    assert np.all(y[swing] == 0)


@pytest.mark.parametrize("mode", list(MODES))
def test_damped_step_matrix(fx, mode):
    b = damped_batch()
    assert input_digest(b, np.arange(len(DAMPED))) == str(fx["digest_damped"]), "generator drifted"
    assert _count(b["contact"])[:len(DAMPED_T)].tolist() == list(DAMPED_T)
    for A in b["Ad"]:
        Nm = A.astype(np.float32) - np.eye(12, dtype=np.float32)
        assert np.any(Nm @ Nm != 0)
    w, st, it, lam = _solve(_plan(mode), b, lam_out=True)
    print("iters", it.tolist())
    ok = _check(b, w, st, fx["w_damped"], 16)
    err = _lam_err(lam, fx["lam_x_damped"], fx["lam_a_damped"])
    assert np.all(err[ok] <= TOL), err


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["light", "heavy", "n5"])
def test_starts(fx, name, mode):
    """Cold, then warm from the cold solve's own w, y and lam, and from non-finite data."""
    N = horizon(name)
    b = batch(name)
    ref = fx[f"w_{name}"]
    plan = _plan(mode, N)
    w0, st0, it0, y0 = _solve(plan, b, y_out=True)
    _check(b, w0, st0, ref, N)
    lam0 = _solve(plan, b, lam_out=True)[3]
    nan_w, nan_y = np.full_like(w0, np.nan), np.full_like(y0, np.inf)
    lx, la = fx[f"lam_x_{name}"], fx[f"lam_a_{name}"]
    yref = y_of(lx, la, b["contact"], N, plan.params.mu)
    stance = _count(b["contact"]) > 0
    # (the y and lam layouts are exclusive in one call: a y start returns y, the others lam)
    for tag, kw in (("w_init", dict(w_init=w0, lam_out=True)),
                    ("w_init + y_init", dict(w_init=w0, y_init=y0, y_out=True)),
                    ("w_init + lam_init", dict(w_init=w0, lam_init=lam0, lam_out=True)),
                    ("lam_init", dict(lam_init=lam0, lam_out=True)),
                    ("non-finite", dict(w_init=nan_w, y_init=nan_y, y_out=True))):
        w, st, it, dual = _solve(plan, b, **kw)
        print(tag, "iters", it.tolist())
        ok = _check(b, w, st, ref, N)
        if "y_out" in kw:
            err = _y_err(dual, yref, lx, la)
            assert np.all(err[ok & stance] <= TOL), (tag, err)
        else:
            err = _lam_err(dual, lx, la)
            assert np.all(err[ok] <= TOL), (tag, err)


@pytest.mark.parametrize("mode", list(MODES))
def test_terrain_and_weights(mode):
    """Per-instance mu / fz_min, then per-instance Q / R, each with one invalid row."""
    plan = _plan(mode)
    ft = load_fixture("qp_terrain.npz")
    b = fixture_batch(ft)
    mu, fz = ft["mu_A"].copy(), ft["fz_min_A"].copy()
    mu[3] = -1.0
    w, st, it, lam = _solve(plan, b, mu=mu, fz_min=fz, lam_out=True)
    ok = _check(b, w, st, ft["w_A"], 16, bad=(3,))
    err = _lam_err(lam, ft["lam_x_A"], ft["lam_a_A"])
    assert np.all(err[ok] <= TOL), err
    fw = load_fixture("qp_weights.npz")
    b = fixture_batch(fw)
    R = fw["R_B"].copy()
    R[5, 2] = 0.0
    w, st, it, lam = _solve(plan, b, Q=fw["Q_B"], R=R, lam_out=True)
    ok = _check(b, w, st, fw["w_B"], 16, bad=(5,))
    assert np.all(lam[5] == 0)
    err = _lam_err(lam, fw["lam_x_B"], fw["lam_a_B"])
    assert np.all(err[ok] <= TOL), err


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["qp_hard.npz", "qp_cfg2.npz"])
def test_sessions(name, mode):
    """Committed fixtures whose solves leave the first session's straight path (the module's
    docstring names the instances and their paths)."""
    f = load_fixture(name)
    b = fixture_batch(f)
    from cmpc import Plan, SolverParams
    plan = Plan(SolverParams(max_batch=len(b["Ad"])))
    plan.set_team(MODES[mode])
    w, st, it, lam = _solve(plan, b, lam_out=True)
    print("iters", it.tolist())
    ok = _check(b, w, st, f["w"], 16)
    err = _lam_err(lam, f["lam_x"], f["lam_a"])
    assert np.all(err[ok] <= TOL), err
