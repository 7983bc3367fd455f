"""GPU: cost and KKT residuals of a batch on the device (cmpc_kkt_run / Plan.kkt,
include/cmpc.h) against oracle.mpc_qp.build_qp + kkt_residuals and cmpc.duals.cost / recover
in float64 NumPy on the same fp32-rounded arrays.

Tolerance (kkt_util): both sides compute the same float64 function and differ only in the order
of their sums, so |dev - ref| <= 1e-12 x S per column, S the largest sum of absolute terms in
any row of that residual; infinities must match exactly."""
import numpy as np
import pytest
import torch

from parity_util import load_fixture
import kkt_util

pytestmark = pytest.mark.gpu
IN = ("Ad", "Bd", "gd", "x0", "xref", "contact")
_cache = {}


def _dev(plan, a):
    return torch.as_tensor(np.ascontiguousarray(a)).contiguous().to(plan.device)


def _run(plan, case, with_lam, idx=None, **over):
    """Plan.kkt on (the instances idx of) a case -> (B, 4) float64 numpy."""
    sel = (lambda a: a) if idx is None else (lambda a: a[idx])
    kw = {k: _dev(plan, sel(case[k])) for k in ("mu", "fz_min", "Q", "R") if k in case}
    kw.update({k: (_dev(plan, v) if isinstance(v, np.ndarray) else v) for k, v in over.items()})
    out = plan.kkt(*[_dev(plan, sel(case[k])) for k in IN], _dev(plan, sel(case["w"])),
                   lam=_dev(plan, sel(case["lam"])) if with_lam else None, **kw)
    torch.cuda.synchronize(plan.device)
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(sel(case["w"])), 4)
    return out.cpu().numpy()


def _fixture(plan, name, tag, with_lam):
    """(case, vals, S) of one fixture set: the reference is computed once per module."""
    key = (name, tag, with_lam)
    if key not in _cache:
        case = kkt_util.fixture_case(load_fixture(name), tag, plan.params)
        _cache[key] = (case,) + kkt_util.case_ref(case, plan.params, with_lam)
    return _cache[key]


def random_case(N, B=67, seed=11):
    """Arbitrary points (nothing is a solution), fp32, with per-instance mu / fz_min / Q / R.
    Instance 0 has no stance leg, instance 1 every leg in stance on every step.  Even instances
    have sign-consistent multipliers (zero wherever the matching bound is infinite: comp is
    finite), odd ones unrestricted multipliers (comp = +inf)."""
    rng = np.random.default_rng(seed + N)
    c = dict(Ad=np.eye(12) + 0.5 * rng.standard_normal((B, 12, 12)),
             Bd=0.1 * rng.standard_normal((B, N, 12, 12)), gd=rng.standard_normal((B, 12)),
             x0=rng.standard_normal((B, 12)), xref=rng.standard_normal((B, N, 12)),
             w=10.0 * rng.standard_normal((B, 24 * N)),
             mu=rng.uniform(0.2, 1.0, B), fz_min=rng.uniform(0.0, 20.0, B),
             Q=rng.uniform(0.0, 50.0, (B, 12)), R=rng.uniform(1e-5, 1e-2, (B, 12)))
    c = {k: kkt_util.f32(v) for k, v in c.items()}
    ct = (rng.random((B, 4, N)) < 0.6).astype(np.uint8)
    ct[0] = 0
    if B > 1:
        ct[1] = 1
    c["contact"] = ct
    lam = rng.standard_normal((B, 52 * N))
    lam[rng.random(lam.shape) < 0.1] = 0.0
    stance = ct.transpose(0, 2, 1).astype(bool)                    # (B, N, 4)
    lx_u = lam[:, 12 * N:24 * N].reshape(B, N, 4, 3)
    lf = lam[:, 36 * N:].reshape(B, N, 4, 4)
    for b in range(0, B, 2):
        lam[b, :12 * N] = 0.0                                      # states: free
        lx_u[b, ..., :2][stance[b]] = 0.0                          # stance fx, fy: free
        lx_u[b, ..., 2][stance[b]] = -np.abs(lx_u[b, ..., 2][stance[b]])  # fz >= fz_min only
        lf[b][stance[b]] = np.abs(lf[b][stance[b]])                # friction rows <= 0 only
        lf[b][~stance[b]] = 0.0                                    # free on a swing leg
    c["lam"] = kkt_util.f32(lam)
    return c


@pytest.mark.parametrize("name,tag", kkt_util.FIXTURES)
def test_fixtures_given_multipliers(plan, name, tag):
    case, vals, S = _fixture(plan, name, tag, True)
    dev = _run(plan, case, True)
    kkt_util.assert_matches(dev, vals, S, f"{name}{tag}")
    # rows filled with the plan's constants give bitwise the result of NULL
    pc = kkt_util.plan_constants(plan.params)
    B = len(dev)
    const = {k: np.full(B, pc[k], np.float32) for k in ("mu", "fz_min") if k not in case}
    const.update({k: np.tile(pc[k].astype(np.float32), (B, 1)) for k in ("Q", "R")
                  if k not in case})
    assert len(const) >= 2
    assert np.array_equal(_run(plan, case, True, **const), dev)
    for k, v in const.items():
        assert np.array_equal(_run(plan, case, True, **{k: v}), dev), k


@pytest.mark.parametrize("name,tag", kkt_util.FIXTURES)
def test_fixtures_recovered_multipliers(plan, name, tag):
    """lam=None: the device recovers the multipliers by the rule of cmpc.duals.recover
    (test_kkt.py guards the face thresholds of these fixtures)."""
    case, vals, S = _fixture(plan, name, tag, False)
    dev = _run(plan, case, False)
    kkt_util.assert_matches(dev, vals, S, f"{name}{tag} recovered")
    assert np.array_equal(_run(plan, case, False, face_tol=None),
                          _run(plan, case, False, face_tol=0.0))
    # another tolerance is honoured: every force 'holds' its faces at tol = 1e3
    tol = float(np.float32(1e3))
    idx = np.arange(0, len(dev), 8)
    v2, S2 = kkt_util.case_ref(case, plan.params, False, tol=tol, idx=idx)
    kkt_util.assert_matches(_run(plan, case, False, idx=idx, face_tol=tol), v2, S2, "tol 1e3")
    assert not np.array_equal(v2, vals[idx])


@pytest.mark.parametrize("N", [1, 5, 16])
def test_arbitrary_points(N):
    from cmpc import Plan, SolverParams
    plan = Plan(SolverParams(N=N, max_batch=8))     # (max_batch does not limit B)
    case = random_case(N)
    for with_lam in (True, False):
        vals, S = kkt_util.case_ref(case, plan.params, with_lam)
        if with_lam:
            inf = np.isinf(vals[:, 3])
            assert not inf[0::2].any() and inf[1::2].all()
        full = None
        for B in (67, 3, 1):
            dev = _run(plan, case, with_lam, idx=np.arange(B))
            kkt_util.assert_matches(dev, vals[:B], S[:B], f"N={N} B={B} lam={with_lam}")
            full = dev if full is None else full
            assert np.array_equal(dev, full[:B])    # independent of B
    plan.close()


def test_invalid_entries_fail_alone(plan):
    case, vals, S = _fixture(plan, "qp_cfg2.npz", "", True)
    idx = np.arange(5)
    pc = kkt_util.plan_constants(plan.params)
    base = dict(mu=np.full(5, pc["mu"], np.float32), fz_min=np.full(5, pc["fz_min"], np.float32),
                Q=np.tile(pc["Q"].astype(np.float32), (5, 1)),
                R=np.tile(pc["R"].astype(np.float32), (5, 1)))
    for with_lam in (True, False):
        good = _run(plan, case, with_lam, idx=idx, **base)
        assert not np.any(np.isnan(good))
        for bad_row, key, where, value in ((2, "mu", (2,), 0.0), (0, "R", (0, 3), 0.0),
                                           (4, "Q", (4, 0), np.nan), (1, "fz_min", (1,), np.inf),
                                           (3, "mu", (3,), np.nan), (3, "Q", (3, 11), -1.0)):
            over = {k: v.copy() for k, v in base.items()}
            over[key][where] = value
            got = _run(plan, case, with_lam, idx=idx, **over)    # (returns: the call is CMPC_OK)
            keep = np.setdiff1d(idx, [bad_row])
            assert np.all(np.isnan(got[bad_row])), (key, got[bad_row])
            assert np.array_equal(got[keep], good[keep]), key


def test_repeatable_and_position_independent(plan):
    case, vals, S = _fixture(plan, "qp_terrain.npz", "_A", True)
    for with_lam in (True, False):
        t = {k: _dev(plan, case[k]) for k in IN + ("w", "lam", "mu", "fz_min")}
        before = {k: v.clone() for k, v in t.items()}

        def run(tt):
            out = plan.kkt(*[tt[k] for k in IN], tt["w"], lam=tt["lam"] if with_lam else None,
                           mu=tt["mu"], fz_min=tt["fz_min"])
            torch.cuda.synchronize(plan.device)
            return out.cpu().numpy()
        a, b = run(t), run(t)
        assert np.array_equal(a, b)
        assert all(torch.equal(t[k], before[k]) for k in t)      # inputs unchanged
        rev = run({k: v.flip(0).contiguous() for k, v in t.items()})
        assert np.array_equal(rev[::-1], a)
        # and a tile of the batch past one grid-stride pass of the kernel (8192 blocks)
        R = 8192 // len(a) + 2
        big = run({k: v.repeat((R,) + (1,) * (v.dim() - 1)).contiguous() for k, v in t.items()})
        assert np.array_equal(big, np.tile(a, (R, 1)))


def test_end_to_end_solve_then_evaluate(plan):
    """64 instances of config 2 solved with lam_out, then evaluated with that lam and with
    recovered multipliers: both match NumPy on the device's own fp32 w / lam."""
    from cmpc import synth, to_device_batch
    d = to_device_batch(synth.make_config(2, B=64), plan.device)
    args = [d[k] for k in IN]
    w, st, it, lam = plan.solve(*args, lam_out=True)
    given, rec = plan.kkt(*args, w, lam=lam), plan.kkt(*args, w)
    torch.cuda.synchronize(plan.device)
    st = st.cpu().numpy()
    assert np.all((st == 1) | (st == 2))
    case = {k: d[k].cpu().numpy() for k in IN}
    case["w"], case["lam"] = w.cpu().numpy(), lam.cpu().numpy()
    for with_lam, dev in ((True, given), (False, rec)):
        vals, S = kkt_util.case_ref(case, plan.params, with_lam)
        dev = dev.cpu().numpy()
        kkt_util.assert_matches(dev, vals, S, f"solve output, lam given={with_lam}")
        print("lam given" if with_lam else "lam recovered", "largest stat over status 1:",
              dev[st == 1, 1].max(), "prim:", dev[st == 1, 2].max(), "comp:", dev[st == 1, 3].max())


def test_graph_capture_reads_w_written_in_place(plan):
    case, vals, S = _fixture(plan, "qp_cfg2.npz", "", True)
    args = [_dev(plan, case[k]) for k in IN]
    w, lam = _dev(plan, case["w"]), _dev(plan, case["lam"])
    w2 = _dev(plan, case["w"][::-1] * np.float32(1.25))
    for with_lam in (True, False):
        w.copy_(_dev(plan, case["w"]))
        out = torch.zeros((len(case["w"]), 4), dtype=torch.float64, device=plan.device)
        s = torch.cuda.Stream(plan.device)
        s.wait_stream(torch.cuda.current_stream(plan.device))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            r = plan.kkt(*args, w, lam=lam if with_lam else None, out=out, stream=s)
        assert r is out
        torch.cuda.current_stream(plan.device).wait_stream(s)
        w.copy_(w2)
        g.replay()
        torch.cuda.synchronize(plan.device)
        got = out.cpu().numpy()
        eager = plan.kkt(*args, w2, lam=lam if with_lam else None)
        torch.cuda.synchronize(plan.device)
        assert np.array_equal(got, eager.cpu().numpy(), equal_nan=True)
        assert not np.array_equal(got[:, 0], vals[:, 0])


def test_closed_loop_report(plan):
    from cmpc.closed_loop import ClosedLoop
    B = 64
    rng = np.random.default_rng(5)
    kw = dict(mu=kkt_util.f32(rng.uniform(0.4, 1.0, B)),
              fz_min=kkt_util.f32(rng.uniform(0.0, 15.0, B)),
              Q=kkt_util.f32(np.asarray(plan.params.Q) * rng.uniform(0.5, 2.0, (B, 12))),
              R=kkt_util.f32(np.asarray(plan.params.R) * rng.uniform(0.5, 2.0, (B, 12))))
    loop = ClosedLoop(B, plan=plan, seed=6, report=True, **kw)
    cmd = np.zeros((B, 4), np.float32)
    cmd[:, 0], cmd[:, 2], cmd[:, 3] = 0.4, 0.27, 1.0
    loop.set_command(cmd)
    assert tuple(loop.kkt.shape) == (B, 4) and loop.kkt.dtype == torch.float64

    def check():
        torch.cuda.synchronize(loop.dev)
        want = plan.kkt(loop.Ad, loop.Bd, loop.gd, loop.x_solve, loop.xref, loop.ct, loop.w,
                        mu=loop.mu, fz_min=loop.fz_min, Q=loop.Q, R=loop.R)
        torch.cuda.synchronize(loop.dev)
        assert torch.equal(loop.kkt, want)
        assert not torch.equal(loop.x_solve, loop.x)             # the plant has moved x on
        st = loop.status.cpu().numpy()
        k = loop.kkt.cpu().numpy()
        assert np.all(np.isfinite(k[(st == 1) | (st == 2)]))
        return k

    ks = []
    for _ in range(3):
        loop.tick()
        ks.append(check())
    loop.capture()
    loop.tick()
    ks.append(check())
    assert not np.array_equal(ks[-1], ks[-2])
    plain = ClosedLoop(B, plan=plan, seed=6, **kw)
    assert plain.report is False and not hasattr(plain, "kkt") and not hasattr(plain, "x_solve")
