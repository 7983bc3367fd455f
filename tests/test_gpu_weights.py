"""GPU: per-instance cost weights (cmpc_solve_io_run's ``Q`` / ``R``, include/cmpc.h) against the
KKT-certified float64 optima of tests/golden/qp_weights.npz (make_golden_weights.py: the 34
instances of qp_terrain.npz, every solve-kernel class; weight set A = Q x exp(U(+-ln 4)), R
log-uniform in [2.5e-6, 1e-4]; set B the wider draw with zeroed Q entries).

Bars (test_gpu_terrain.py's): status-1 answers within 1e-4 of the optimum, a status-2 answer
within 1e-3, at most one status 2 per 34 instances; feasibility to 1e-3 N and X within 1e-4 of
the float64 rollout; multipliers to the bound of tests/test_gpu_duals.py.
"""
import numpy as np
import pytest
import torch

from parity_util import load_fixture, fixture_batch, rel_err_U, split_w, rollout64, feasibility

pytestmark = pytest.mark.gpu
TOL = 1e-4
TOL_ST2 = 1e-3
Q0 = np.array([1, 1, 50, 10, 20, 1, 2, 2, 1, 1, 1, 1], np.float32)     # the plan's constants
R0 = np.full(12, 1e-5, np.float32)


@pytest.fixture(scope="module")
def fx():
    return load_fixture("qp_weights.npz")


def _dev(plan, a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).contiguous().to(plan.device)


def _solve(plan, batch, Q=None, R=None, **kw):
    """numpy batch + numpy weights (and options) in, tuple of numpy arrays out."""
    from cmpc import to_device_batch
    d = to_device_batch(batch, plan.device)
    kw = {k: (_dev(plan, v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    r = plan.solve(d["Ad"], d["Bd"], d["gd"], d["x0"], d["xref"], d["contact"],
                   Q=None if Q is None else _dev(plan, Q), R=None if R is None else _dev(plan, R),
                   **kw)
    torch.cuda.synchronize(plan.device)
    return tuple(t.cpu().numpy() for t in r)


def _tile(fx, tag, n):
    """The fixture n times over, copy after copy: neighbours hold different weights."""
    batch = {k: np.tile(v, (n,) + (1,) * (v.ndim - 1)) for k, v in fixture_batch(fx).items()}
    return (batch, np.tile(fx[f"Q_{tag}"], (n, 1)), np.tile(fx[f"R_{tag}"], (n, 1)),
            np.tile(fx[f"w_{tag}"], (n, 1)))


def _assert_parity(batch, w_ref, w, st, max_st2, mu=0.8, fz_min=10.0):
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
    feas = feasibility(b64, U, mu=mu, fz_min=fz_min)
    assert feas.max() < 1e-3, (feas.max(), int(feas.argmax()))
    Xr = rollout64(b64, U)
    assert np.max(np.abs(X - Xr)) < 1e-4, np.max(np.abs(X - Xr))


def test_parity_team_kernel(plan, fx):
    """34 instances with weights of their own, one batch below the team bound.  With the plan's
    constant weights every one of these optima is at least 18 % away."""
    assert 34 <= plan.team_batch()
    batch, Q, R, w_ref = _tile(fx, "A", 1)
    w, st, it = _solve(plan, batch, Q, R)
    _assert_parity(batch, w_ref, w, st, max_st2=1)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_parity_group_kernels(plan, fx, tag):
    """Past the team bound: the one-wave-per-QP kernels of all three register classes."""
    n = plan.team_batch() // 34 + 1
    batch, Q, R, w_ref = _tile(fx, tag, n)
    assert len(Q) > plan.team_batch() and all(plan.solve_kernels(len(Q)))
    w, st, it = _solve(plan, batch, Q, R)
    _assert_parity(batch, w_ref, w, st, max_st2=n)


def test_reference_multipliers_with_weights(plan, fx):
    """lam_out holds the KKT multipliers of each instance's own QP, to the bound of
    test_gpu_duals.py::test_device_multipliers_match_certified."""
    from oracle import mpc_qp
    batch = fixture_batch(fx)
    Q, R = fx["Q_A"], fx["R_A"]
    w, st, it, lam = _solve(plan, batch, Q, R, lam_out=True)
    assert np.all((st == 1) | (st == 2)) and np.sum(st == 2) <= 1
    w64, lam64 = w.astype(np.float64), lam.astype(np.float64)
    ref = np.concatenate([fx["lam_x_A"], fx["lam_a_A"]], axis=1)
    lerr = np.max(np.abs(lam64 - ref), axis=1) / np.maximum(np.max(np.abs(ref), axis=1), 1e-9)
    print("max multiplier error", lerr[st == 1].max())
    assert lerr[st == 1].max() <= TOL, (lerr.max(), int(lerr.argmax()))
    for i in np.flatnonzero(st == 1)[::4]:           # and they are KKT multipliers of w
        b = {k: np.asarray(batch[k][i], np.float64) for k in ("Ad", "Bd", "gd", "x0", "xref")}
        qp = mpc_qp.build_qp(b["Ad"], b["Bd"], b["gd"], b["x0"], b["xref"].T, batch["contact"][i],
                             Q=Q[i].astype(np.float64), R=R[i].astype(np.float64))
        k = mpc_qp.kkt_residuals(qp, w64[i], lam64[i, :384], lam64[i, 384:])
        assert k["prim"] < 1e-3 and k["stat"] < 1e-3 * (1 + np.max(np.abs(qp["g"]))), (i, k)


@pytest.mark.parametrize("B", [512, 2048])     # team kernel, group kernels
def test_null_and_constant_arrays_are_bit_identical(plan, B):
    from cmpc import Plan, SolverParams, synth
    batch = synth.make_config(2, B=B)
    assert (B <= plan.team_batch()) == (B == 512)
    Qc, Rc = np.tile(Q0, (B, 1)), np.tile(R0, (B, 1))
    base = _solve(plan, batch)
    for other in (_solve(plan, batch, Q=None, R=None), _solve(plan, batch, Qc, Rc),
                  _solve(plan, batch, Q=Qc), _solve(plan, batch, R=Rc),
                  # (through the struct entry with NULL Q / R: the terrain arrays route there)
                  _solve(plan, batch, mu=np.full(B, 0.8, np.float32))):
        for a, b in zip(base, other):
            assert np.array_equal(a, b)
    Q1 = (Q0 * np.array([2, 0.5, 0.5, 1, 3, 1, 1, 0.25, 4, 1, 2, 1], np.float32)).astype(np.float32)
    R1 = (R0 * np.array([4, 1, 0.5, 2, 8, 0.25, 1, 1, 3, 1, 0.5, 6], np.float32)).astype(np.float32)
    other = Plan(SolverParams(Q=tuple(float(v) for v in Q1), R=tuple(float(v) for v in R1),
                              max_batch=B))
    want = _solve(other, batch)
    got = _solve(plan, batch, np.tile(Q1, (B, 1)), np.tile(R1, (B, 1)))
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    assert not np.array_equal(want[0], base[0])


def test_invalid_rows_fail_alone(plan):
    from cmpc import synth
    B = 64
    batch = synth.make_config(2, B=B)
    wt = synth.make_weights(B, seed=9)
    Q, R = wt["Q"].astype(np.float32), wt["R"].astype(np.float32)
    good = _solve(plan, batch, Q, R, y_out=True)
    bad_Q, bad_R = Q.copy(), R.copy()
    bad_Q[3, 7] = np.nan
    bad_Q[17, 0] = -1.0
    bad_R[18, 11] = 0.0
    bad_R[40, 4] = np.inf
    bad_R[63, 2] = np.nan
    bad = [3, 17, 18, 40, 63]
    w, st, it, y = _solve(plan, batch, bad_Q, bad_R, y_out=True)    # (returns: the call is CMPC_OK)
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
    # the reference's multipliers: a zero row too, the others as without the bad rows
    gl = _solve(plan, batch, Q, R, lam_out=True)
    wl, stl, itl, lam = _solve(plan, batch, bad_Q, bad_R, lam_out=True)
    assert np.all(stl[bad] == -10) and np.all(lam[bad] == 0.0)
    for a, b in zip(gl, (wl, stl, itl, lam)):
        assert np.array_equal(a[keep], b[keep])


def test_weights_combine_with_terrain(plan, fx):
    """Set A weights and qp_terrain's set A terrain together, against an optimum certified here
    by the oracle: one instance per solve-kernel class and one more."""
    from oracle import mpc_qp, active_set
    ft = load_fixture("qp_terrain.npz")
    nf = 3 * (fx["contact"] != 0).reshape(34, -1).sum(1)
    idx = [int(np.flatnonzero(nf <= 128)[0]), int(np.flatnonzero((nf > 128) & (nf <= 160))[0]),
           int(np.flatnonzero(nf > 160)[0]), int(np.flatnonzero(nf <= 128)[-1])]
    assert len(set(idx)) == 4
    batch = {k: v[idx] for k, v in fixture_batch(fx).items()}
    Q, R = fx["Q_A"][idx], fx["R_A"][idx]
    mu, fz = ft["mu_A"][idx], ft["fz_min_A"][idx]
    w, st, it = _solve(plan, batch, Q, R, mu=mu, fz_min=fz)
    w_ref = []
    for j in range(4):
        b = {k: np.asarray(batch[k][j], np.float64) for k in ("Ad", "Bd", "gd", "x0", "xref")}
        qp = mpc_qp.build_qp(b["Ad"], b["Bd"], b["gd"], b["x0"], b["xref"].T, batch["contact"][j],
                             Q=Q[j].astype(np.float64), R=R[j].astype(np.float64),
                             mu=float(mu[j]), fz_min=float(fz[j]))
        # (the answer only seeds the active set: a certified point is the unique optimum)
        r = active_set.certified_optimum(qp, w[j].astype(np.float64))
        assert max(r["kkt"].values()) <= 1e-8, (idx[j], r["kkt"])
        w_ref.append(r["w"])
    _assert_parity(batch, np.array(w_ref), w, st, max_st2=1,
                   mu=mu.astype(np.float64)[:, None, None], fz_min=fz.astype(np.float64)[:, None, None])


def test_graph_replay_reads_weights_written_in_place(plan, fx):
    from cmpc import to_device_batch
    batch = fixture_batch(fx)
    d = to_device_batch(batch, plan.device)
    Q, R = _dev(plan, fx["Q_A"]), _dev(plan, fx["R_A"])
    N = plan.params.N
    out = (torch.empty((34, 24 * N), dtype=torch.float32, device=plan.device),
           torch.empty((34,), dtype=torch.int32, device=plan.device),
           torch.empty((34,), dtype=torch.int32, device=plan.device))
    args = (d["Ad"], d["Bd"], d["gd"], d["x0"], d["xref"], d["contact"])
    plan.solve(*args, out=out, Q=Q, R=R)            # (eager once, as ClosedLoop.capture does)
    torch.cuda.synchronize(plan.device)
    s = torch.cuda.Stream(plan.device)
    s.wait_stream(torch.cuda.current_stream(plan.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.solve(*args, out=out, stream=s, Q=Q, R=R)
    torch.cuda.current_stream(plan.device).wait_stream(s)
    g.replay()
    torch.cuda.synchronize(plan.device)
    wA, stA = out[0].cpu().numpy(), out[1].cpu().numpy()
    _assert_parity(batch, fx["w_A"], wA, stA, max_st2=1)
    Q.copy_(_dev(plan, fx["Q_B"]))                  # in place: the graph holds the pointers
    R.copy_(_dev(plan, fx["R_B"]))
    g.replay()
    torch.cuda.synchronize(plan.device)
    got = tuple(t.cpu().numpy() for t in out)
    want = _solve(plan, batch, fx["Q_B"], fx["R_B"])
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    _assert_parity(batch, fx["w_B"], got[0], got[1], max_st2=1)


def test_weight_change_across_a_warm_tick(plan, fx):
    """Every robot is re-weighted (set A -> set B) between two warm-started ticks, and back: the
    previous tick's point and dual belong to another objective."""
    batch = fixture_batch(fx)
    wA, stA, itA, yA = _solve(plan, batch, fx["Q_A"], fx["R_A"], y_out=True)
    _assert_parity(batch, fx["w_A"], wA, stA, max_st2=1)
    wB, stB, itB, yB = _solve(plan, batch, fx["Q_B"], fx["R_B"], w_init=wA, y_init=yA, y_out=True)
    _assert_parity(batch, fx["w_B"], wB, stB, max_st2=1)
    wA2, stA2, itA2, yA2 = _solve(plan, batch, fx["Q_A"], fx["R_A"], w_init=wB, y_init=yB,
                                  y_out=True)
    _assert_parity(batch, fx["w_A"], wA2, stA2, max_st2=1)


def test_closed_loop_reads_weights_written_between_ticks(plan):
    """Twin loops with per-robot weights walk alike; a row of loop.Q written in place re-weights
    that robot from the next tick of the captured graph on."""
    from cmpc import synth
    from cmpc.closed_loop import ClosedLoop
    B = 64
    wt = synth.make_weights(B, seed=4)
    a, b = (ClosedLoop(B, plan=plan, seed=3, Q=wt["Q"], R=wt["R"]) for _ in range(2))
    assert a.Q.shape == (B, 12) and a.Q.dtype == torch.float32 and a.R.is_cuda
    cmd = np.zeros((B, 4), np.float32)
    cmd[:, 0] = 0.4
    cmd[:, 2] = 0.27
    cmd[:, 3] = 1.0
    a.set_command(cmd)
    b.set_command(cmd)

    def tick():
        a.tick()
        b.tick()
        torch.cuda.synchronize(a.dev)
        for loop in (a, b):
            st = loop.status.cpu().numpy()
            assert np.all((st == 1) | (st == 2)), st

    for _ in range(2):
        tick()
    a.capture()
    b.capture()
    for _ in range(2):
        tick()
    assert torch.equal(a.w, b.w) and torch.equal(a.x, b.x)
    changed = np.arange(B) % 2 == 0
    Q2 = wt["Q"].astype(np.float32)
    Q2[changed] = Q2[changed] * np.array([1, 1, 4, 4, 4, 1, 1, 1, 0.25, 1, 1, 1], np.float32)
    a.Q.copy_(torch.as_tensor(Q2, device=a.dev))   # in place: the graph holds the pointer
    tick()
    N = a.N
    dU = (a.w[:, 12 * N:] - b.w[:, 12 * N:]).abs().amax(dim=1).cpu().numpy()
    # (the twins are bit-identical up to here and a tick is deterministic, so any difference is
    # the re-weighting, and no difference on the other robots shows that rows do not mix)
    print("max |dU| of the re-weighted robots: min", dU[changed].min(), "max", dU[changed].max())
    assert np.all(dU[changed] > 0.0), dU[changed].min()
    assert np.all(dU[~changed] == 0.0), dU[~changed].max()
