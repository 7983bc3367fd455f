"""GPU: per-instance friction coefficient and stance normal-force floor (cmpc_solve_io_run's
``mu`` / ``fz_min``, include/cmpc.h) against the KKT-certified float64 optima of
tests/golden/qp_terrain.npz (make_golden_terrain.py: 34 instances of every solve-kernel class,
terrain set A ~ U(0.2, 1.0) x U(0, 20) and set B with mu ~ U(0.2, 0.5)).

Bars: status-1 answers within 1e-4 of the optimum (the north star), a status-2 answer within
1e-3, at most one status 2 per 34 instances (parity_util.assert_verified's rule for a small
batch); feasibility to 1e-3 N and X within 1e-4 of the float64 rollout, as the plan-wide
parity tests; multipliers to the bound of tests/test_gpu_duals.py.
"""
import numpy as np
import pytest
import torch

from parity_util import load_fixture, fixture_batch, rel_err_U, split_w, rollout64, feasibility

pytestmark = pytest.mark.gpu
TOL = 1e-4
TOL_ST2 = 1e-3


@pytest.fixture(scope="module")
def fx():
    return load_fixture("qp_terrain.npz")


def _dev(plan, a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).contiguous().to(plan.device)


def _solve(plan, batch, mu=None, fz_min=None, **kw):
    """numpy batch + numpy terrain in, tuple of float64 / int numpy arrays out."""
    from cmpc import to_device_batch
    d = to_device_batch(batch, plan.device)
    kw = {k: (_dev(plan, v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    r = plan.solve(d["Ad"], d["Bd"], d["gd"], d["x0"], d["xref"], d["contact"],
                   mu=None if mu is None else _dev(plan, mu),
                   fz_min=None if fz_min is None else _dev(plan, fz_min), **kw)
    torch.cuda.synchronize(plan.device)
    return tuple(t.cpu().numpy() for t in r)


def _tile(fx, tag, R):
    """The fixture R times over, copy after copy: neighbours hold different terrain."""
    batch = {k: np.tile(v, (R,) + (1,) * (v.ndim - 1)) for k, v in fixture_batch(fx).items()}
    return batch, np.tile(fx[f"mu_{tag}"], R), np.tile(fx[f"fz_min_{tag}"], R), np.tile(fx[f"w_{tag}"], (R, 1))


def _assert_parity(batch, mu, fz, w_ref, w, st, max_st2):
    w = w.astype(np.float64)
    err = rel_err_U(w, w_ref)
    print("status", dict(zip(*np.unique(st, return_counts=True))), "max rel err st1",
          err[st == 1].max(initial=0.0), "st2", err[st == 2].max(initial=0.0))
    assert np.all((st == 1) | (st == 2)), np.unique(st, return_counts=True)
    assert np.sum(st == 2) <= max_st2, np.flatnonzero(st == 2)
    assert err[st == 1].max(initial=0.0) <= TOL, (err.max(), int(np.where(st == 1, err, 0).argmax()))
    assert err[st == 2].max(initial=0.0) <= TOL_ST2, np.flatnonzero((st == 2) & (err > TOL_ST2))
    X, U = split_w(w)
    b64 = {k: np.asarray(v, np.float64) if k != "contact" else v for k, v in batch.items()}
    feas = feasibility(b64, U, mu=mu.astype(np.float64)[:, None, None],
                       fz_min=fz.astype(np.float64)[:, None, None])
    assert feas.max() < 1e-3, (feas.max(), int(feas.argmax()))
    Xr = rollout64(b64, U)
    assert np.max(np.abs(X - Xr)) < 1e-4, np.max(np.abs(X - Xr))


def test_parity_team_kernel(plan, fx):
    """34 instances with a terrain each, one batch below the team bound.  On a solver whose
    friction is a plan constant 7 of 8 such optima are 8-56 % away."""
    assert 34 <= plan.team_batch()
    batch, mu, fz, w_ref = _tile(fx, "A", 1)
    w, st, it = _solve(plan, batch, mu, fz)
    _assert_parity(batch, mu, fz, w_ref, w, st, max_st2=1)


def test_parity_group_kernels(plan, fx):
    """Past the team bound: the one-wave-per-QP kernels of all three register classes."""
    R = plan.team_batch() // 34 + 1
    batch, mu, fz, w_ref = _tile(fx, "A", R)
    assert len(mu) > plan.team_batch() and all(plan.solve_kernels(len(mu)))
    w, st, it = _solve(plan, batch, mu, fz)
    _assert_parity(batch, mu, fz, w_ref, w, st, max_st2=R)


@pytest.mark.parametrize("B", [512, 2048])     # team kernel, group kernels
def test_null_and_constant_arrays_are_bit_identical(plan, B):
    from cmpc import Plan, SolverParams, synth
    batch = synth.make_config(2, B=B)
    assert (B <= plan.team_batch()) == (B == 512)
    base = _solve(plan, batch)
    none = _solve(plan, batch, mu=None, fz_min=None)
    for a, b in zip(base, none):
        assert np.array_equal(a, b)
    const = _solve(plan, batch, np.full(B, 0.8, np.float32), np.full(B, 10.0, np.float32))
    for a, b in zip(base, const):
        assert np.array_equal(a, b)
    only_mu = _solve(plan, batch, mu=np.full(B, 0.8, np.float32))
    for a, b in zip(base, only_mu):
        assert np.array_equal(a, b)
    other = Plan(SolverParams(mu=0.35, fz_min=5.0, max_batch=B))
    want = _solve(other, batch)
    got = _solve(plan, batch, np.full(B, 0.35, np.float32), np.full(B, 5.0, np.float32))
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    assert not np.array_equal(want[0], base[0])


def test_invalid_entries_fail_alone(plan):
    from cmpc import synth
    B = 64
    batch = synth.make_config(2, B=B)
    t = synth.make_terrain(B, seed=9)
    mu, fz = t["mu"].astype(np.float32), t["fz_min"].astype(np.float32)
    good = _solve(plan, batch, mu, fz, y_out=True)
    bad_mu, bad_fz = mu.copy(), fz.copy()
    bad_mu[[3, 17, 18, 40]] = [np.nan, 0.0, -0.5, np.inf]
    bad_fz[63] = np.nan
    bad = [3, 17, 18, 40, 63]
    w, st, it, y = _solve(plan, batch, bad_mu, bad_fz, y_out=True)   # (returns: the call is CMPC_OK)
    assert np.all(st[bad] == -10), st[bad]
    X, U = split_w(w.astype(np.float64))
    assert np.all(U[bad] == 0.0) and np.all(np.isfinite(w[bad])) and np.all(y[bad] == 0.0)
    b64 = {k: np.asarray(v, np.float32).astype(np.float64) if k != "contact" else v
           for k, v in batch.items() if k in ("Ad", "Bd", "gd", "x0", "xref", "contact")}
    Xr = rollout64(b64, np.zeros_like(U))
    assert np.max(np.abs(X[bad] - Xr[bad])) < 1e-4
    keep = np.setdiff1d(np.arange(B), bad)
    for a, b in zip(good, (w, st, it, y)):
        assert np.array_equal(a[keep], b[keep])
    assert np.all((good[1] == 1) | (good[1] == 2))


def test_terrain_change_across_a_warm_tick(plan, fx):
    """Every robot steps onto ice (set A -> set B) between two warm-started ticks, and back: the
    previous tick's faces belong to another pyramid and must not be accepted as they are."""
    batch = fixture_batch(fx)
    wA, stA, itA, yA = _solve(plan, batch, fx["mu_A"], fx["fz_min_A"], y_out=True)
    assert np.all((stA == 1) | (stA == 2))
    wB, stB, itB, yB = _solve(plan, batch, fx["mu_B"], fx["fz_min_B"], w_init=wA, y_init=yA,
                              y_out=True)
    _assert_parity(batch, fx["mu_B"], fx["fz_min_B"], fx["w_B"], wB, stB, max_st2=1)
    wA2, stA2, itA2, yA2 = _solve(plan, batch, fx["mu_A"], fx["fz_min_A"], w_init=wB, y_init=yB,
                                  y_out=True)
    _assert_parity(batch, fx["mu_A"], fx["fz_min_A"], fx["w_A"], wA2, stA2, max_st2=1)


def test_reference_multipliers_with_terrain(plan, fx):
    """lam_out holds KKT multipliers of each instance's own QP (the bound of
    test_gpu_duals.py::test_device_multipliers_match_certified), and warm-starting from them and
    the returned point polishes directly (iters 0), as test_warm_start_from_reference_multipliers
    expects of the plan-wide case."""
    from oracle import mpc_qp
    batch = fixture_batch(fx)
    mu, fz = fx["mu_A"], fx["fz_min_A"]
    w, st, it, lam = _solve(plan, batch, mu, fz, lam_out=True)
    assert np.all((st == 1) | (st == 2)) and np.sum(st == 2) <= 1
    w64, lam64 = w.astype(np.float64), lam.astype(np.float64)
    for i in np.flatnonzero(st == 1):
        b = {k: np.asarray(batch[k][i], np.float64) for k in ("Ad", "Bd", "gd", "x0", "xref")}
        qp = mpc_qp.build_qp(b["Ad"], b["Bd"], b["gd"], b["x0"], b["xref"].T, batch["contact"][i],
                             mu=float(mu[i]), fz_min=float(fz[i]))
        k = mpc_qp.kkt_residuals(qp, w64[i], lam64[i, :384], lam64[i, 384:])
        assert k["prim"] < 1e-3 and k["stat"] < 1e-3 * (1 + np.max(np.abs(qp["g"]))), (i, k)
    ref = np.concatenate([fx["lam_x_A"], fx["lam_a_A"]], axis=1)
    lerr = np.max(np.abs(lam64 - ref), axis=1) / np.maximum(np.max(np.abs(ref), axis=1), 1e-9)
    assert lerr[st == 1].max() <= TOL, (lerr.max(), int(lerr.argmax()))
    w2, st2, it2, lam2 = _solve(plan, batch, mu, fz, w_init=w, lam_init=lam, lam_out=True)
    ok = st == 1
    assert np.all(st2[ok] == 1) and int(it2[ok].max()) == 0, (st2, it2)
    assert rel_err_U(w2, fx["w_A"])[ok].max() <= TOL


def test_closed_loop_reads_terrain_written_between_replays():
    from cmpc.closed_loop import ClosedLoop
    B = 64
    mu0 = np.where(np.arange(B) % 2 == 0, 0.2, 0.9).astype(np.float32)
    loop = ClosedLoop(B, mu=mu0, fz_min=np.full(B, 10.0, np.float32))
    cmd = np.zeros((B, 4), np.float32)
    cmd[:, 2] = 0.27
    cmd[:, 3] = 2.0                                  # yaw-rate command: needs tangential force
    loop.set_command(cmd)
    N = loop.N
    ice = np.arange(B) % 2 == 0

    def check():
        torch.cuda.synchronize(loop.dev)
        st = loop.status.cpu().numpy()
        assert np.all((st == 1) | (st == 2)), st
        U = loop.w[:, 12 * N:].cpu().numpy().astype(np.float64)
        F = U[:, :12].reshape(B, 4, 3)
        stance = loop.ct[:, :, 0].cpu().numpy() != 0
        mu = loop.mu.cpu().numpy().astype(np.float64)[:, None]
        fzm = loop.fz_min.cpu().numpy().astype(np.float64)[:, None]
        tol = 1e-3 * np.abs(U).max(axis=1)[:, None]
        fx_, fy_, fz_ = F[..., 0], F[..., 1], F[..., 2]
        viol = np.maximum.reduce([fzm - fz_, np.abs(fx_) - mu * fz_, np.abs(fy_) - mu * fz_])
        assert np.all(np.where(stance, viol, 0.0) <= tol), np.where(stance, viol, 0.0).max()
        assert np.all(np.abs(F[~stance]) == 0.0)
        ratio = np.where(stance, np.maximum(np.abs(fx_), np.abs(fy_)) / np.maximum(fz_, 1e-9), 0.0)
        return ratio.max(axis=1)

    def yaw_rate(wz):
        cmd[:, 3] = wz
        loop.set_command(cmd)                        # (in place too: the graph reads the command)

    for _ in range(2):
        loop.tick()
        check()
    loop.capture()
    # The plant follows a yaw-rate step within a tick or two (after which no tangential force is
    # needed), so each phase starts with a reversal of the command: braking 4 rad/s of yaw rate
    # saturates mu = 0.2 (the float64 oracle holds all four feet at |f_t| = 0.2 fz for half that
    # step) and stays well inside mu = 0.9.
    yaw_rate(-2.0)
    before = 0.0
    for _ in range(4):
        loop.tick()
        before = max(before, float(check()[ice].max()))
    assert before > 0.19, before                     # on the face (check() bounds it from above)
    loop.mu.fill_(0.9)                               # in place: the graph holds the pointer
    yaw_rate(2.0)
    seen = 0.0
    for _ in range(4):
        loop.tick()
        seen = max(seen, float(check()[ice].max()))
    # (0.21: clear of what the pyramid tolerance lets a robot still held at mu = 0.2 reach)
    assert seen > 0.21, (before, seen)
