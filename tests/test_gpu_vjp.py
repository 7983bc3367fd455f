"""GPU: gradients of a loss through a solved batch (cmpc_vjp_run / Plan.vjp / cmpc.autograd,
include/cmpc.h) against the two float64 NumPy references of tests/vjp_util.py on the same
fp32-rounded arrays.

Bar (vjp_util): |dev - ref| <= 1e-8 x S per output, S the defining formula with every factor
replaced by its absolute value; where S is 0 the device value must be exactly 0.  Every instance
is held to it against reference (b), the kernel's route in NumPy, and a subset against (a), the
dense KKT solve, which test_vjp.py ties to (b) within 1e-9 x S and to central differences.

Measured on an MI355X: the worst ratio to the bar is 7.4e-4 against (a) and 4.1e-4 against (b) on
every set but one -- instance 51 of qp_cfg2 is at 0.954 of the bar in g_xref (0.118 in g_Ad, 0.057
in g_Q) against both references: with R = 1e-5 its adjoint forces are ~1e5 along directions that
barely move the state, and dx = sum Bd du cancels by that factor."""
import ctypes

import numpy as np
import pytest
import torch

import gain_util
import kkt_util
import vjp_util
from test_gpu_gain import random_case, _fixture, _dev

pytestmark = pytest.mark.gpu
IN = ("Ad", "Bd", "gd", "x0", "xref", "contact")
ALL = vjp_util.OUTPUTS
_gw = {}


def _vjp(plan, case, gw, idx=None, want=ALL, use_w=True, faces=None, **over):
    """Plan.vjp on (the instances idx of) a case -> dict of numpy arrays."""
    sel = (lambda a: a) if idx is None else (lambda a: a[idx])
    kw = {k: _dev(plan, sel(case[k])) for k in ("mu", "fz_min", "Q", "R") if k in case}
    kw.update(over)
    out = plan.vjp(*[_dev(plan, sel(case[k])) for k in IN], _dev(plan, sel(gw)),
                   w=_dev(plan, sel(case["w"])) if use_w else None,
                   faces=None if faces is None else _dev(plan, sel(faces)), want=want, **kw)
    torch.cuda.synchronize(plan.device)
    B, N = len(sel(case["Ad"])), case["Bd"].shape[1]
    assert set(out) == set(want)
    for n, t in out.items():
        assert tuple(t.shape) == vjp_util.shapes(B, N)[n] and t.dtype == torch.float64, n
    return {n: t.cpu().numpy() for n, t in out.items()}


def _fixture_gw(plan, name, tag):
    case, faces = _fixture(plan, name, tag)
    if (name, tag) not in _gw:
        _gw[(name, tag)] = vjp_util.random_gw(np.random.default_rng(17), case["w"].shape)
    return case, faces, _gw[(name, tag)]


def _check(dev, case, faces, gw, params, rows, dense_rows, what):
    """Instances `rows` of dev against reference (b), `dense_rows` also against (a); prints the
    worst ratio per output and reference before asserting."""
    worst = {"a": {n: 0.0 for n in ALL}, "b": {n: 0.0 for n in ALL}}
    for i in rows:
        iv = kkt_util.instance_values(case, i, params)
        args, kw = gain_util.instance_args(case, i, iv)
        mine = {n: dev[n][i] for n in ALL if n in dev}
        assert all(np.all(np.isfinite(v)) for v in mine.values()), (what, i)
        refs = [("b", vjp_util.ref_riccati(*args, faces[i], gw=gw[i], **kw))]
        if i in dense_rows:
            refs.append(("a", vjp_util.ref_dense(*args, faces[i], gw=gw[i], **kw)))
        for tag, (vals, S) in refs:
            for n, r in vjp_util.worst_ratio(mine, vals, S, vjp_util.TOL_REL).items():
                worst[tag][n] = max(worst[tag][n], r)
    print(what, "worst |dev - ref| / (1e-8 S): dense KKT (a)", worst["a"], "riccati (b)", worst["b"])
    assert max(worst["a"].values()) <= 1.0 and max(worst["b"].values()) <= 1.0, (what, worst)


@pytest.mark.parametrize("name,tag", kkt_util.FIXTURES)
def test_fixtures_faces_from_w(plan, name, tag):
    """The five fixture sets with their per-instance mu / fz_min / Q / R, faces read off w, all
    nine outputs; (b) on every instance, (a) on every fourth."""
    case, faces, gw = _fixture_gw(plan, name, tag)
    dev = _vjp(plan, case, gw)
    B = len(faces)
    _check(dev, case, faces, gw, plan.params, range(B), set(range(0, B, 4)), f"{name}{tag}")
    # the faces given back, and any subset of the outputs, are bitwise the same
    again = _vjp(plan, case, gw, use_w=False, faces=faces)
    assert all(np.array_equal(again[n], dev[n]) for n in ALL)
    for want in [(n,) for n in ALL] + [("x0", "xref"), ("xref", "Q", "R"), ("mu", "Bd"),
                                       ("fz_min", "gd", "R")]:
        sub = _vjp(plan, case, gw, want=want)
        assert all(np.array_equal(sub[n], dev[n]) for n in want), want


@pytest.mark.parametrize("N", [1, 5, 16])
def test_arbitrary_face_sets_given(N):
    from cmpc import Plan, SolverParams, _lib
    plan = Plan(SolverParams(N=N, max_batch=8))     # (max_batch does not limit B)
    c, faces, nan_rows = random_case(N)
    B = len(faces)
    gw = vjp_util.random_gw(np.random.default_rng(31 + N), (B, 24 * N))
    good = [i for i in range(B) if i not in nan_rows]
    dev = _vjp(plan, c, gw, use_w=False, faces=faces)
    for n in ALL:
        assert np.all(np.isnan(dev[n][nan_rows])), n
        assert np.all(np.isfinite(dev[n][good])), n
    dense = set(range(0, B, 4)) | {0, 1, 2}
    _check(dev, c, faces, gw, plan.params, good, dense & set(good), f"N={N} B={B}")
    # smaller batches of the same instances: bitwise the same rows (independent of B and place)
    for idx in ([2, 5, 6], [0], [5], [3]):
        idx = np.array(idx)
        sub = _vjp(plan, c, gw, idx=idx, use_w=False, faces=faces)
        for n in ALL:
            assert np.array_equal(sub[n], dev[n][idx], equal_nan=True), (n, idx)
    # a struct that stops after g_x0: g_x0 is computed, nothing past it is written
    t = {k: _dev(plan, c[k]) for k in IN + ("mu", "fz_min", "Q", "R")}
    t["faces"], t["gw"] = _dev(plan, faces), _dev(plan, gw)
    g = torch.zeros((B, 12), dtype=torch.float64, device=plan.device)
    guard = torch.full((B, N, 12, 12), 7.0, dtype=torch.float64, device=plan.device)
    io = _lib.CVjpIO()
    for k, v in t.items():
        setattr(io, k, v.data_ptr())
    io.g_x0 = g.data_ptr()
    for n in ALL[1:]:
        setattr(io, "g_" + n, guard.data_ptr())
    io.size = _lib.CVjpIO.g_x0.offset + ctypes.sizeof(ctypes.c_void_p)
    with torch.cuda.device(plan.device):
        rc = plan.lib.cmpc_vjp_run(plan._h, ctypes.c_int64(B), ctypes.byref(io), ctypes.c_void_p(
            torch.cuda.current_stream(plan.device).cuda_stream))
    torch.cuda.synchronize(plan.device)
    assert rc == 0, _lib.last_error(plan.lib)
    assert np.array_equal(g.cpu().numpy(), dev["x0"], equal_nan=True)
    assert torch.all(guard == 7.0)
    plan.close()


def test_x0_gradient_of_a_force_is_a_row_of_the_gain(plan):
    """gw = e_{12N + i}: g_x0 = d u_0[i] / d x0 = row i of Plan.gain's K, on 16 instances of
    qp_cfg2, within 2e-8 x max(1, max|K|) (each side's own bar)."""
    case, faces = _fixture(plan, "qp_cfg2.npz", "")
    idx = np.arange(0, 64, 4)
    N = plan.params.N
    t = [_dev(plan, case[k][idx]) for k in IN]
    fc = _dev(plan, faces[idx])
    K = plan.gain(*t, faces=fc)["K"].cpu().numpy()
    worst = 0.0
    for i in range(12):
        gw = np.zeros((len(idx), 24 * N), np.float32)
        gw[:, 12 * N + i] = 1.0
        g = plan.vjp(*t, _dev(plan, gw), faces=fc, want=("x0",))["x0"].cpu().numpy()
        worst = max(worst, float(np.max(np.abs(g - K[:, i, :]).max(axis=1) /
                                        (2e-8 * np.maximum(1.0, np.abs(K).max(axis=(1, 2)))))))
    print("worst |g_x0 - K[i]| / (2e-8 max(1, max|K|)):", worst)
    assert worst <= 1.0


def test_linear_in_xref_gd_x0(plan):
    """With the faces fixed u_star is affine in (xref, gd, x0): for a gw without a state part
    gw_u . (u_star(theta + d) - u_star(theta)) = g_theta . d, for displacements that are not
    small.  Tolerance: the sum of the two bars -- each u_star within 1e-8 x max|u| of its exact
    value, weighed by |gw_u|_1, and g_theta within 1e-8 x S_theta, weighed by |d|_1."""
    case, faces, gw_all = _fixture_gw(plan, "qp_cfg2.npz", "")
    idx = np.arange(0, 64, 4)
    N = plan.params.N
    gw = gw_all.copy()
    gw[:, :12 * N] = 0.0
    names = ("xref", "gd", "x0")
    base = _vjp(plan, case, gw, idx=idx, use_w=False, faces=faces, want=names)
    S = []
    for i in idx:
        iv = kkt_util.instance_values(case, i, plan.params)
        args, kw = gain_util.instance_args(case, i, iv)
        S.append(vjp_util.ref_riccati(*args, faces[i], gw=gw[i], **kw)[1])

    def u_star(c):
        out = plan.gain(*[_dev(plan, c[k][idx]) for k in IN], faces=_dev(plan, faces[idx]),
                        want=("K", "u_star"))["u_star"]
        return out.cpu().numpy()
    u0 = u_star(case)
    gu = gw[idx][:, 12 * N:].astype(np.float64)
    rng = np.random.default_rng(9)
    worst = 0.0
    for size in (0.05, 0.5, 3.0):
        for n in names:
            moved = dict(case)
            moved[n] = case[n].copy()
            moved[n][idx] = kkt_util.f32(case[n][idx] + size * rng.uniform(-1.0, 1.0, case[n][idx].shape))
            d = (moved[n][idx].astype(np.float64) - case[n][idx].astype(np.float64)).reshape(len(idx), -1)
            assert np.abs(d).max() > 0.5 * size
            u1 = u_star(moved)
            lhs = np.sum(gu * (u1 - u0), axis=1)
            rhs = np.sum(base[n].reshape(len(idx), -1) * d, axis=1)
            umax = np.maximum(np.abs(u1).max(axis=1), np.abs(u0).max(axis=1))
            tol = vjp_util.TOL_REL * (2.0 * umax * np.abs(gu).sum(axis=1) +
                                      np.array([s[n] for s in S]) * np.abs(d).sum(axis=1))
            ratio = np.abs(lhs - rhs) / tol
            print("size", size, n, "max |g . d|", np.abs(rhs).max(), "worst / tol", ratio.max())
            worst = max(worst, ratio.max())
    assert worst <= 1.0


def test_repeatable_and_position_independent(plan):
    case, faces, gw = _fixture_gw(plan, "qp_terrain.npz", "_A")
    a, b = _vjp(plan, case, gw), _vjp(plan, case, gw)
    assert all(np.array_equal(a[n], b[n]) for n in ALL)
    rev = {k: (v[::-1].copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    r = _vjp(plan, rev, gw[::-1].copy())
    assert all(np.array_equal(r[n][::-1], a[n]) for n in ALL)
    perm = np.random.default_rng(1).permutation(len(faces))
    p = _vjp(plan, case, gw, idx=perm)
    assert all(np.array_equal(p[n], a[n][perm]) for n in ALL)
    # and a tile of the batch past one grid-stride pass of the kernel (8192 blocks)
    reps = 8192 // len(faces) + 2
    tile = lambda v: np.tile(v, (reps,) + (1,) * (v.ndim - 1))  # noqa: E731
    big = _vjp(plan, {k: tile(v) for k, v in case.items() if isinstance(v, np.ndarray)}, tile(gw),
               want=("x0", "Q", "mu", "fz_min", "Ad"))
    assert all(np.array_equal(v, tile(a[n])) for n, v in big.items())


def test_autograd_layer(plan):
    """cmpc.autograd.solve on 64 instances of config 2 with per-robot mu, fz_min, Q, R requiring
    a gradient: L = (c . w).sum(); torch.autograd.grad equals Plan.vjp's outputs cast to fp32."""
    from cmpc import autograd, synth, to_device_batch
    B, N = 64, plan.params.N
    d = to_device_batch(synth.make_config(2, B=B), plan.device)
    args = [d[k] for k in IN]
    p = plan.params
    f32 = dict(dtype=torch.float32, device=plan.device)
    per = dict(mu=torch.full((B,), p.mu, **f32), fz_min=torch.full((B,), p.fz_min, **f32),
               Q=torch.tensor(p.Q, **f32).repeat(B, 1), R=torch.tensor(p.R, **f32).repeat(B, 1))
    per["mu"][3] = -1.0                                    # an invalid entry: status -10
    for t in per.values():
        t.requires_grad_(True)
    x0 = args[3].clone().requires_grad_(True)
    call = args[:3] + [x0] + args[4:]
    w, st, it = autograd.solve(plan, *call, **per)
    assert w.requires_grad and not st.requires_grad and not it.requires_grad
    assert int(st[3]) == -10 and bool(torch.all(st[torch.arange(B) != 3] > 0))
    c = torch.randn(w.shape, generator=torch.Generator().manual_seed(2)).to(plan.device)
    loss = (c * w).sum()
    leaves = [per[n] for n in ("mu", "fz_min", "Q", "R")] + [x0]
    grads = torch.autograd.grad(loss, leaves, retain_graph=False)
    ref = plan.vjp(*[a.detach() for a in call], c, w=w.detach(),
                   **{n: t.detach() for n, t in per.items()},
                   want=("mu", "fz_min", "Q", "R", "x0"))
    torch.cuda.synchronize(plan.device)
    for g, n, leaf in zip(grads, ("mu", "fz_min", "Q", "R", "x0"), leaves):
        want = ref[n].to(torch.float32)
        assert bool(torch.isnan(want[3]).all())             # the entry's own answer there: NaN
        want[3] = 0.0                                       # the layer's: no gradient
        assert g.dtype == leaf.dtype and g.shape == leaf.shape and torch.equal(g, want), n
        assert bool(torch.all(torch.isfinite(g))) and float(g.abs().max()) > 0.0, n
    # inputs that do not require a gradient get None (x0 among them this time), and a second
    # backward raises
    asked = []
    vjp = plan.vjp
    plan.vjp = lambda *a, **k: asked.append(tuple(k["want"])) or vjp(*a, **k)
    try:
        w2, _, _ = autograd.solve(plan, *args, **per)
        w2.backward(c)
    finally:
        del plan.vjp
    assert asked == [("mu", "fz_min", "Q", "R")]           # exactly what needs a gradient
    assert all(a.grad is None for a in args)
    assert torch.equal(per["Q"].grad, grads[2]) and torch.equal(per["mu"].grad, grads[0])
    with pytest.raises(RuntimeError):
        w2.backward(c)


def test_graph_capture(plan):
    """One Plan.vjp call captured in a torch.cuda.graph, replayed on a changed gw: bitwise the
    eager call."""
    case, faces, gw = _fixture_gw(plan, "qp_cfg2.npz", "")
    B, N = len(faces), plan.params.N
    t = [_dev(plan, case[k]) for k in IN]
    w = _dev(plan, case["w"])
    g1, g2 = _dev(plan, gw), _dev(plan, vjp_util.random_gw(np.random.default_rng(4), gw.shape))
    buf = g1.clone()
    out = {n: torch.empty(s, dtype=torch.float64, device=plan.device)
           for n, s in vjp_util.shapes(B, N).items()}
    side = torch.cuda.Stream(plan.device)
    side.wait_stream(torch.cuda.current_stream(plan.device))
    with torch.cuda.stream(side):
        plan.vjp(*t, buf, w=w, want=ALL, out=out)           # (warm-up on the capture stream)
    torch.cuda.current_stream(plan.device).wait_stream(side)
    torch.cuda.synchronize(plan.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.vjp(*t, buf, w=w, want=ALL, out=out)
    buf.copy_(g2)
    for v in out.values():
        v.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize(plan.device)
    eager = plan.vjp(*t, g2, w=w, want=ALL)
    torch.cuda.synchronize(plan.device)
    first = plan.vjp(*t, g1, w=w, want=("x0",))["x0"]
    assert all(torch.equal(out[n], eager[n]) for n in ALL)
    assert not torch.equal(first, eager["x0"])
