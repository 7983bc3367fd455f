"""GPU: gradients and tangents of the dynamics builder on the device (cmpc_dynamics_vjp_run /
cmpc_dynamics_jvp_run, Plan.dynamics_vjp / Plan.dynamics_jvp, cmpc.autograd.build_dynamics)
against dyn_grad_util's float64 references.

Inputs are the first B robots and N steps of synth.make_config(3, B=8197); gradients and
tangents are random.  Bars: the vjp within 1e-12 x S per robot and output (each entry a sum of
at most 64 terms of fewer than 40 fp64 roundings, the 3x3 inverse at cond < 50, device sin / cos
within a few ulps: ~2e-14 x S expected); the jvp within one fp32 rounding 2^-23 |ref| plus
1e-12 x S.  Shapes: N = 16 fills all 64 lanes, N = 5 and N = 1 leave padded lanes, B = 8197
passes the 8192-block grid cap into the grid-stride loop.

Measured on an MI355X, worst ratio to the bar over all shapes: vjp 6.4e-4
(g_r_feet at N = 16, B = 8197), jvp 0.4995 (the half-ulp of its fp32 rounding), the adjoint
identity between the entries 0.033, the fp64 chain 2.5e-4."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dyn_grad_util as dg

pytestmark = pytest.mark.gpu

SHAPES = [(16, 1), (16, 67), (5, 1), (5, 67), (1, 1), (1, 67), (16, 8197)]
IN = ("mass", "inertia", "r_feet", "xref")


@functools.lru_cache(maxsize=None)
def _base():
    from cmpc import synth
    return synth.make_config(3, B=8197)


@functools.lru_cache(maxsize=None)
def _case(N, B):
    """The case of a shape with both references, computed once and shared (not modified)."""
    c = dg.random_case(np.random.default_rng(1000 * N + B), B, N, _base())
    vjp = dg.ref_vjp(*dg.inputs(c), c["g_Ad"], c["g_Bd"])
    jvp = dg.ref_jvp(*dg.inputs(c), *[c["d_" + k] for k in IN])
    return c, vjp, jvp


_plans = {}


def _plan_for(plan, N):
    """The session's plan at its horizon, else one plan per horizon (max_batch does not limit B)."""
    from cmpc import Plan, SolverParams
    if N == plan.params.N:
        return plan
    if N not in _plans:
        _plans[N] = Plan(SolverParams(N=N, max_batch=8))
    return _plans[N]


def _dev(plan, a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(plan.device)


def _args(plan, c):
    return [_dev(plan, c[k]) for k in IN] + [c["dt"]]


def _grads(plan, c):
    return dict(g_Ad=_dev(plan, c["g_Ad"]), g_Bd=_dev(plan, c["g_Bd"]))


def _tangents(plan, c):
    return {k: _dev(plan, c["d_" + k]) for k in IN}


def _host(res):
    return {n: t.cpu().numpy() for n, t in res.items()}


@pytest.mark.parametrize("N,B", SHAPES)
def test_vjp_against_reference(plan, N, B):
    p = _plan_for(plan, N)
    c, (vals, S), _ = _case(N, B)
    res = p.dynamics_vjp(*_args(p, c), **_grads(p, c))
    torch.cuda.synchronize(p.device)
    got = _host(res)
    assert set(got) == set(dg.VJP_OUTPUTS)
    assert all(got[n].dtype == np.float64 and got[n].shape == vals[n].shape for n in got)
    worst = dg.worst_ratio(got, vals, S)
    print(f"N={N} B={B} worst |dev - ref| / (1e-12 S):", worst)
    assert all(np.all(s > 0.0) for s in S.values())
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("N,B", SHAPES)
def test_jvp_against_reference(plan, N, B):
    p = _plan_for(plan, N)
    c, _, (vals, S) = _case(N, B)
    res = p.dynamics_jvp(*_args(p, c), _tangents(p, c))
    torch.cuda.synchronize(p.device)
    got = _host(res)
    assert set(got) == {"Ad", "Bd"} and all(v.dtype == np.float32 for v in got.values())
    worst = dg.worst_ratio(got, vals, S, rel=dg.REL32)
    print(f"N={N} B={B} worst |dev - ref| / (2^-23 |ref| + 1e-12 S):", worst)
    assert max(worst.values()) <= 1.0, worst
    const = np.ones((12, 12), bool)
    const[3:5, 9:11] = False
    assert np.all(got["Ad"][:, const] == 0.0)             # the constant entries: exactly 0
    assert np.abs(got["Ad"]).max() > 0.0 and np.abs(got["Bd"]).max() > 0.0


def test_adjoint_identity_between_the_entries(plan):
    """<g_Ad, d_Ad> + <g_Bd, d_Bd> with the device's fp32 d_Ad, d_Bd against g . d with the
    device's gradients, per robot.  The bar is what the two tests above allow each entry:
    2^-23 sum |g_i| |d_i| over the left side for the fp32 rounding, plus 1e-12 x (sum |g_i| S_i
    on the left, sum S_i |d_i| on the right)."""
    N, B = 16, 67
    c, (_, Sv), (_, Sj) = _case(N, B)
    g = _host(plan.dynamics_vjp(*_args(plan, c), **_grads(plan, c)))
    d = _host(plan.dynamics_jvp(*_args(plan, c), _tangents(plan, c)))
    torch.cuda.synchronize(plan.device)
    rows = lambda x: np.asarray(x, np.float64).reshape(B, -1)                # noqa: E731
    dot = lambda x, y: (rows(x) * rows(y)).sum(1)                            # noqa: E731
    mag = lambda x: np.abs(rows(x)).sum(1)                                   # noqa: E731
    dyaw = dg.f32(c["d_xref"])[:, :, 5].sum(1) / N
    left = dot(c["g_Ad"], d["Ad"]) + dot(c["g_Bd"], d["Bd"])
    right = (dot(g["mass"], c["d_mass"]) + dot(g["inertia"], c["d_inertia"]) +
             dot(g["r_feet"], c["d_r_feet"]) + dot(g["yaw"], dyaw))
    bar = (dg.REL32 * (dot(np.abs(c["g_Ad"]), np.abs(d["Ad"])) + dot(np.abs(c["g_Bd"]), np.abs(d["Bd"]))) +
           dg.TOL * (mag(c["g_Ad"]) * Sj["Ad"] + mag(c["g_Bd"]) * Sj["Bd"] +
                     Sv["mass"] * mag(c["d_mass"]) + Sv["inertia"] * mag(c["d_inertia"]) +
                     Sv["r_feet"] * mag(c["d_r_feet"]) + Sv["yaw"] * np.abs(dyaw)))
    ratio = np.abs(left - right) / bar
    print("worst adjoint mismatch / bar:", float(ratio.max()))
    assert np.all(np.abs(left) > 0.0) and ratio.max() <= 1.0


def test_subsets_and_null_inputs(plan):
    """An output asked for alone is bitwise the one asked for with all the others; a NULL
    gradient or tangent gives the values of an array of zeros (==: the sign of a zero may
    differ)."""
    N, B = 5, 67
    p = _plan_for(plan, N)
    c, _, _ = _case(N, B)
    a, g, t = _args(p, c), _grads(p, c), _tangents(p, c)
    every = p.dynamics_vjp(*a, **g)
    for n in dg.VJP_OUTPUTS:
        alone = p.dynamics_vjp(*a, **g, want=(n,))
        assert set(alone) == {n} and torch.equal(alone[n], every[n]), n
    pair = p.dynamics_vjp(*a, **g, want=("r_feet", "yaw"))
    assert torch.equal(pair["r_feet"], every["r_feet"]) and torch.equal(pair["yaw"], every["yaw"])
    both = p.dynamics_jvp(*a, t)
    for n in dg.JVP_OUTPUTS:
        alone = p.dynamics_jvp(*a, t, want=(n,))
        assert set(alone) == {n} and torch.equal(alone[n], both[n]), n
    for n in ("g_Ad", "g_Bd"):
        null = p.dynamics_vjp(*a, **dict(g, **{n: None}))
        zero = p.dynamics_vjp(*a, **dict(g, **{n: torch.zeros_like(g[n])}))
        for o in dg.VJP_OUTPUTS:
            assert bool((null[o] == zero[o]).all()), (n, o)
        assert not torch.equal(null["yaw"], every["yaw"])
    for n in IN:
        null = p.dynamics_jvp(*a, {k: v for k, v in t.items() if k != n})
        zero = p.dynamics_jvp(*a, dict(t, **{n: torch.zeros_like(t[n])}))
        for o in dg.JVP_OUTPUTS:
            assert bool((null[o] == zero[o]).all()), (n, o)
        assert not torch.equal(null["Bd"], both["Bd"]) or not torch.equal(null["Ad"], both["Ad"])
    torch.cuda.synchronize(p.device)


def test_repeatable_and_position_independent(plan):
    """The batch twice, and once in a permuted order: bitwise-equal rows."""
    N, B = 16, 67
    c, _, _ = _case(N, B)
    a, g, t = _args(plan, c), _grads(plan, c), _tangents(plan, c)
    perm = torch.as_tensor(np.random.default_rng(7).permutation(B)).to(plan.device)
    take = lambda x: x[perm].contiguous()                                    # noqa: E731
    ap = [take(x) for x in a[:4]] + [a[4]]
    v1, v2 = plan.dynamics_vjp(*a, **g), plan.dynamics_vjp(*a, **g)
    vp = plan.dynamics_vjp(*ap, **{n: take(x) for n, x in g.items()})
    j1, j2 = plan.dynamics_jvp(*a, t), plan.dynamics_jvp(*a, t)
    jp = plan.dynamics_jvp(*ap, {n: take(x) for n, x in t.items()})
    torch.cuda.synchronize(plan.device)
    for first, again, moved in ((v1, v2, vp), (j1, j2, jp)):
        for n in first:
            assert torch.equal(first[n], again[n]), n
            assert torch.equal(first[n][perm], moved[n]), n


def test_fp64_chain_and_autograd_wiring(plan):
    """64 robots of config 2.  Plan.vjp(want=Ad, Bd) -> Plan.dynamics_vjp stays in float64 and
    matches ref_vjp of the downloaded g_Ad, g_Bd; autograd.build_dynamics -> autograd.solve ->
    backward hands each input the same launches' results through the same casts, exactly; under
    forward_ad the tangent of Bd is Plan.dynamics_jvp's."""
    import torch.autograd.forward_ad as fwAD
    from cmpc import autograd, synth, to_device_batch
    B, N = 64, plan.params.N
    b = synth.make_config(2, B=B)
    d = to_device_batch(b, plan.device)
    f32 = torch.float32
    m, I, r, xr = (_dev(plan, np.float32(b[k])) for k in ("m", "I_world", "r_legs", "xref"))
    dt = float(b["dt"])
    assert torch.equal(xr, d["xref"])
    Ad, Bd, gd = plan.build_dynamics(m, I, r, xr, dt)
    rest = [d["x0"], d["xref"], d["contact"]]
    w, st, _ = plan.solve(Ad, Bd, gd, *rest)
    assert bool((st > 0).all())
    gen = torch.Generator().manual_seed(9)
    cw = torch.randn(B, 24 * N, generator=gen).to(plan.device)
    # the chain that stays in float64
    s64 = plan.vjp(Ad, Bd, gd, *rest, cw, w=w, want=("Ad", "Bd"))
    got = plan.dynamics_vjp(m, I, r, xr, dt, g_Ad=s64["Ad"], g_Bd=s64["Bd"])
    torch.cuda.synchronize(plan.device)
    vals, S = dg.ref_vjp(m.cpu().numpy(), I.cpu().numpy(), r.cpu().numpy(), xr.cpu().numpy(), dt,
                         s64["Ad"].cpu().numpy(), s64["Bd"].cpu().numpy())
    worst = dg.worst_ratio(_host(got), vals, S)
    print("fp64 chain, worst |dev - ref| / (1e-12 S):", worst)
    assert max(worst.values()) <= 1.0, worst
    # the autograd layer
    leaves = [t.clone().requires_grad_(True) for t in (m, I, r, xr)]
    asked = []
    dvjp = plan.dynamics_vjp
    plan.dynamics_vjp = lambda *a, **k: asked.append(tuple(k["want"])) or dvjp(*a, **k)
    try:
        A2, B2, g2 = autograd.build_dynamics(plan, *leaves, dt)
        assert not g2.requires_grad and A2.requires_grad and B2.requires_grad
        assert torch.equal(A2, Ad) and torch.equal(B2, Bd) and torch.equal(g2, gd)
        w2, st2, _ = autograd.solve(plan, A2, B2, g2, d["x0"], leaves[3], d["contact"])
        (w2 * cw).sum().backward()
    finally:
        del plan.dynamics_vjp
    assert asked == [("mass", "inertia", "r_feet", "yaw")]
    assert torch.equal(w2.detach(), w)
    s32 = plan.vjp(Ad, Bd, gd, *rest, cw, w=w, want=("Ad", "Bd", "xref"))
    exp = plan.dynamics_vjp(m, I, r, xr, dt, g_Ad=s32["Ad"].to(f32).to(torch.float64),
                            g_Bd=s32["Bd"].to(f32).to(torch.float64))
    for leaf, n in zip(leaves[:3], ("mass", "inertia", "r_feet")):
        assert leaf.grad.dtype == f32 and torch.equal(leaf.grad, exp[n].to(f32)), n
        assert float(leaf.grad.abs().max()) > 0.0 and bool(torch.isfinite(leaf.grad).all()), n
    spread = torch.zeros_like(xr)
    spread[:, :, 5] = (exp["yaw"] / N).to(f32)[:, None]
    assert float(spread.abs().max()) > 0.0
    assert torch.equal(leaves[3].grad, s32["xref"].to(f32) + spread)
    # forward mode
    tan = (0.1 * torch.randn(B, N, 4, 3, generator=gen)).to(plan.device)
    with fwAD.dual_level():
        A3, B3, g3 = autograd.build_dynamics(plan, m, I, fwAD.make_dual(r, tan), xr, dt)
        tB = fwAD.unpack_dual(B3).tangent
        tA = fwAD.unpack_dual(A3).tangent
        assert fwAD.unpack_dual(g3).tangent is None
        ref = plan.dynamics_jvp(m, I, r, xr, dt, dict(r_feet=tan))
        assert torch.equal(tB, ref["Bd"]) and float(tB.abs().max()) > 0.0
        assert tA is None or torch.equal(tA, ref["Ad"])
        A4, B4, _ = autograd.build_dynamics(plan, m, I, r, xr, dt)    # no tangent: nothing moves
        assert fwAD.unpack_dual(B4).tangent is None and fwAD.unpack_dual(A4).tangent is None
    torch.cuda.synchronize(plan.device)


def test_graph_capture(plan):
    """Both entries captured on one stream at B = 64, one after the other, replayed once: bitwise
    the eager results."""
    N, B = plan.params.N, 64
    c = dg.random_case(np.random.default_rng(3), B, N, _base())
    a, g, t = _args(plan, c), _grads(plan, c), _tangents(plan, c)
    f64 = dict(dtype=torch.float64, device=plan.device)
    vout = dict(mass=torch.empty(B, **f64), inertia=torch.empty(B, 3, 3, **f64),
                r_feet=torch.empty(B, N, 4, 3, **f64), yaw=torch.empty(B, **f64))
    jout = dict(Ad=torch.empty(B, 12, 12, device=plan.device),
                Bd=torch.empty(B, N, 12, 12, device=plan.device))

    def both():
        plan.dynamics_vjp(*a, **g, out=vout)
        plan.dynamics_jvp(*a, t, out=jout)

    side = torch.cuda.Stream(plan.device)
    side.wait_stream(torch.cuda.current_stream(plan.device))
    with torch.cuda.stream(side):
        both()                                             # (warm-up on the capture stream)
    torch.cuda.current_stream(plan.device).wait_stream(side)
    torch.cuda.synchronize(plan.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for o in list(vout.values()) + list(jout.values()):
        o.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize(plan.device)
    ev, ej = plan.dynamics_vjp(*a, **g), plan.dynamics_jvp(*a, t)
    torch.cuda.synchronize(plan.device)
    for n in vout:
        assert torch.equal(vout[n], ev[n]) and bool((vout[n] != -1.0).any()), n
    for n in jout:
        assert torch.equal(jout[n], ej[n]), n


def _raw(plan, entry, mirror, B, size=None, handle=True, **fields):
    """One call of ``entry`` with the mirror's fields set -> (rc, message)."""
    from cmpc import _lib
    io = mirror()
    io.size = ctypes.sizeof(mirror) if size is None else size
    for k, v in fields.items():
        setattr(io, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    with torch.cuda.device(plan.device):
        rc = getattr(plan.lib, entry)(plan._h if handle else None, B, ctypes.byref(io), None)
    return rc, _lib.last_error(plan.lib)


def test_validation(plan):
    from cmpc import CmpcError, _lib
    N, B = plan.params.N, 3
    c = dg.random_case(np.random.default_rng(4), B, N, _base())
    a, g, t = _args(plan, c), _grads(plan, c), _tangents(plan, c)
    ins = dict(zip(IN, a[:4]))
    out = plan.dynamics_vjp(*a, **g)
    jo = plan.dynamics_jvp(*a, t)
    cases = (("cmpc_dynamics_vjp_run", _lib.CDynamicsVjpIO, "g_mass",
              dict(ins, dt=a[4], g_Ad=g["g_Ad"], g_Bd=g["g_Bd"], g_mass=out["mass"]),
              ("g_Ad", "g_Bd"), ("g_mass",)),
             ("cmpc_dynamics_jvp_run", _lib.CDynamicsJvpIO, "d_Ad",
              dict(ins, dt=a[4], d_mass=t["mass"], d_Ad=jo["Ad"]), ("d_mass",), ("d_Ad",)))
    for entry, mirror, first, ok, given, outputs in cases:
        assert _raw(plan, entry, mirror, B, **ok)[0] == 0
        assert _raw(plan, entry, mirror, 0, **ok)[0] == 0                    # B == 0 returns
        assert _raw(plan, entry, mirror, 0, **dict(ok, mass=None))[0] == 0
        bad = [dict(handle=False), dict(B=-1), dict(size=getattr(mirror, first).offset), dict(size=4)]
        bad += [dict(dt=v) for v in (0.0, -0.01, float("nan"), float("inf"))]
        bad += [{n: None} for n in IN]
        bad += [{n: None for n in given}, {n: None for n in outputs}]
        for change in bad:
            kw = dict(ok, **{k: v for k, v in change.items() if k not in ("handle", "B", "size")})
            rc, msg = _raw(plan, entry, mirror, change.get("B", B), size=change.get("size"),
                           handle=change.get("handle", True), **kw)
            assert rc == -22 and entry in msg, (entry, change, rc, msg)
    # a struct that ends after the first output reads the outputs past it as NULL
    ends = dict(cases[0][3], g_mass=None, g_yaw=out["yaw"])
    rc, msg = _raw(plan, "cmpc_dynamics_vjp_run", _lib.CDynamicsVjpIO, B,
                   size=_lib.CDynamicsVjpIO.g_inertia.offset, **ends)
    assert rc == -22 and "every output is null" in msg
    # the Python layer
    for dt in (0.0, -0.01, float("nan")):
        with pytest.raises((CmpcError, ValueError)):
            plan.dynamics_vjp(*a[:4], dt, **g)
        with pytest.raises((CmpcError, ValueError)):
            plan.dynamics_jvp(*a[:4], dt, t)
    with pytest.raises(ValueError):
        plan.dynamics_vjp(*a)
    with pytest.raises(ValueError):
        plan.dynamics_vjp(*a, **g, want=())
    with pytest.raises(ValueError):
        plan.dynamics_vjp(*a, **g, want=("xref",))
    with pytest.raises(ValueError):
        plan.dynamics_jvp(*a, {})
    with pytest.raises(ValueError):
        plan.dynamics_jvp(*a, dict(gd=t["mass"]))
    with pytest.raises(ValueError):
        plan.dynamics_jvp(*a, t, want=())
    with pytest.raises((TypeError, ValueError)):
        plan.dynamics_vjp(*a, g_Ad=g["g_Ad"].to(torch.float32))
    with pytest.raises((TypeError, ValueError)):
        plan.dynamics_jvp(*a, dict(mass=t["mass"].to(torch.float64)))
    # B == 0 returns
    e = [x[:0].contiguous() for x in a[:4]] + [a[4]]
    r0 = plan.dynamics_vjp(*e, g_Bd=g["g_Bd"][:0].contiguous())
    j0 = plan.dynamics_jvp(*e, dict(mass=t["mass"][:0].contiguous()))
    assert r0["r_feet"].shape == (0, N, 4, 3) and j0["Bd"].shape == (0, N, 12, 12)
    torch.cuda.synchronize(plan.device)
