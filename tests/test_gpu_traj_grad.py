"""GPU: gradients and tangents of the trajectory generator on the device (cmpc_traj_vjp_run /
cmpc_traj_jvp_run, Plan.traj_vjp / Plan.traj_jvp, cmpc.autograd.generate_traj) against
traj_grad_util's float64 references.

Inputs are synth.make_tick_inputs(B, seed=1000 N + B, mixed=True, N=N); gradients and tangents
are standard normal.  Bars: the vjp within 1e-12 x S per robot and output (dyn_grad_util.TOL's
derivation: sums of at most 64 terms of fewer than 40 fp64 roundings, device sin / cos within a
few ulps); the jvp's fp32 outputs within one fp32 rounding 2^-23 |ref| plus 1e-12 x S, its fp64
d_pos_des_out within 1e-12 x S.  Shapes: N = 16 fills all 64 lanes, N = 5 and N = 1 leave padded
lanes, B = 8197 passes the 8192-block grid cap into the grid-stride loop.

Measured on an MI355X, worst ratio to the bar over all shapes: vjp 3.6e-4
(g_foot_lever at N = 16, B = 8197), the jvp's fp32 outputs 0.49998 (the half-ulp of their one
rounding) and its d_pos_des_out 0 (equal), the adjoint identity between the entries 0.062, g_yaw
given against g_yaw / N spread by hand 0 (equal), the fp64 chain 2.9e-4."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import traj_grad_util as tg

pytestmark = pytest.mark.gpu

SHAPES = [(16, 1), (16, 67), (5, 1), (5, 67), (1, 1), (1, 67), (16, 8197)]
IN = tg.INPUTS


@functools.lru_cache(maxsize=None)
def _case(N, B):
    """The case of a shape with both references, computed once and shared (not modified)."""
    c = tg.random_case(np.random.default_rng(1000 * N + B), B, N)
    vjp = tg.ref_vjp(*tg.inputs(c), **tg.gradients(c))
    jvp = tg.ref_jvp(*tg.inputs(c), **tg.tangents(c))
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
    return {k: _dev(plan, c[k]) for k in ("g_xref", "g_r_feet", "g_yaw", "g_pos_des")}


def _tangents(plan, c):
    return {k: _dev(plan, c["d_" + k]) for k in tg.JVP_TANGENTS}


def _host(res):
    return {n: t.cpu().numpy() for n, t in res.items()}


@pytest.mark.parametrize("N,B", SHAPES)
def test_vjp_against_reference(plan, N, B):
    p = _plan_for(plan, N)
    c, (vals, S), _ = _case(N, B)
    a = _args(p, c)
    before = a[1].clone()
    res = p.traj_vjp(*a, **_grads(p, c))
    torch.cuda.synchronize(p.device)
    got = _host(res)
    assert set(got) == set(tg.VJP_OUTPUTS) and torch.equal(a[1], before)
    assert all(got[n].dtype == np.float64 and got[n].shape == vals[n].shape for n in got)
    worst = tg.worst_ratio(got, vals, S)
    print(f"N={N} B={B} worst |dev - ref| / (1e-12 S):", worst)
    assert np.all(S["x0"] > 0.0) and np.all(S["cmd"] > 0.0)
    assert max(worst.values()) <= 1.0, worst
    assert np.all(got["x0"][:, [2, 6, 7, 8, 9, 10, 11]] == 0.0) and np.all(got["pos_des"][:, 2] == 0.0)


@pytest.mark.parametrize("N,B", SHAPES)
def test_jvp_against_reference(plan, N, B):
    p = _plan_for(plan, N)
    c, _, (vals, S) = _case(N, B)
    res = p.traj_jvp(*_args(p, c), _tangents(p, c))
    torch.cuda.synchronize(p.device)
    got = _host(res)
    assert set(got) == set(tg.JVP_OUTPUTS)
    assert got["xref"].dtype == got["r_feet"].dtype == np.float32 and got["pos_des"].dtype == np.float64
    f32s = {n: got[n] for n in ("xref", "r_feet")}
    worst = tg.worst_ratio(f32s, vals, S, rel=tg.REL32)
    worst.update(tg.worst_ratio(dict(pos_des=got["pos_des"]), vals, S))
    print(f"N={N} B={B} worst |dev - ref| / (2^-23 |ref| + 1e-12 S; pos_des 1e-12 S):", worst)
    assert max(worst.values()) <= 1.0, worst
    cls, _ = tg.classes(c["t_now"], c["gait"], c["dt"], N)
    assert np.all(got["r_feet"][cls == tg.SWING] == 0.0)            # swing levers: exactly 0
    assert np.all(got["xref"][:, :, [3, 4, 8, 9, 10]] == 0.0)
    assert np.abs(got["xref"]).max() > 0.0 and (B == 1 or np.abs(got["r_feet"]).max() > 0.0)


def test_adjoint_identity_between_the_entries(plan):
    """<G, d_xref> + <H, d_r_feet> + <gp, d_pos_des'> with the device's tangents against g . d
    with the device's gradients, per robot.  The bar is what the two tests above allow each entry:
    2^-23 sum |g_i| |d_i| over the fp32 outputs for their rounding, plus 1e-12 x (sum |g_i| S_i on
    the left, sum S_i |d_i| on the right)."""
    N, B = 16, 67
    c, (_, Sv), (_, Sj) = _case(N, B)
    g = _host(plan.traj_vjp(*_args(plan, c), **_grads(plan, c)))
    d = _host(plan.traj_jvp(*_args(plan, c), _tangents(plan, c)))
    torch.cuda.synchronize(plan.device)
    rows = lambda x: np.asarray(x, np.float64).reshape(B, -1)                # noqa: E731
    dot = lambda x, y: (rows(x) * rows(y)).sum(1)                            # noqa: E731
    mag = lambda x: np.abs(rows(x)).sum(1)                                   # noqa: E731
    G = c["g_xref"].copy()
    G[:, :, 5] += (c["g_yaw"] / N)[:, None]
    left = dot(G, d["xref"]) + dot(c["g_r_feet"], d["r_feet"]) + dot(c["g_pos_des"], d["pos_des"])
    right = sum(dot(g[n], c["d_" + n]) for n in tg.JVP_TANGENTS)
    bar = (tg.REL32 * (dot(np.abs(G), np.abs(d["xref"])) + dot(np.abs(c["g_r_feet"]), np.abs(d["r_feet"]))) +
           tg.TOL * (mag(G) * Sj["xref"] + mag(c["g_r_feet"]) * Sj["r_feet"] +
                     mag(c["g_pos_des"]) * Sj["pos_des"] +
                     sum(Sv[n] * mag(c["d_" + n]) for n in tg.JVP_TANGENTS)))
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
    every = p.traj_vjp(*a, **g)
    for n in tg.VJP_OUTPUTS:
        alone = p.traj_vjp(*a, **g, want=(n,))
        assert set(alone) == {n} and torch.equal(alone[n], every[n]), n
    pair = p.traj_vjp(*a, **g, want=("cmd", "foot_lever"))
    assert torch.equal(pair["cmd"], every["cmd"]) and torch.equal(pair["foot_lever"], every["foot_lever"])
    allj = p.traj_jvp(*a, t)
    for n in tg.JVP_OUTPUTS:
        alone = p.traj_jvp(*a, t, want=(n,))
        assert set(alone) == {n} and torch.equal(alone[n], allj[n]), n
    for n in g:
        null = p.traj_vjp(*a, **dict(g, **{n: None}))
        zero = p.traj_vjp(*a, **dict(g, **{n: torch.zeros_like(g[n])}))
        for o in tg.VJP_OUTPUTS:
            assert bool((null[o] == zero[o]).all()), (n, o)
        assert any(not torch.equal(null[o], every[o]) for o in tg.VJP_OUTPUTS), n
    for n in t:
        null = p.traj_jvp(*a, {k: v for k, v in t.items() if k != n})
        zero = p.traj_jvp(*a, dict(t, **{n: torch.zeros_like(t[n])}))
        for o in tg.JVP_OUTPUTS:
            assert bool((null[o] == zero[o]).all()), (n, o)
        assert any(not torch.equal(null[o], allj[o]) for o in tg.JVP_OUTPUTS), n
    torch.cuda.synchronize(p.device)


def test_g_yaw_is_spread_over_the_steps(plan):
    """g_yaw given equals g_yaw / N added into column 5 of g_xref by hand, within 1e-12 x S."""
    N, B = 16, 67
    c, (_, S), _ = _case(N, B)
    a, g = _args(plan, c), _grads(plan, c)
    given = plan.traj_vjp(*a, **g)
    byhand = g["g_xref"].clone()
    byhand[:, :, 5] += (g["g_yaw"] / N)[:, None]
    spread = plan.traj_vjp(*a, **dict(g, g_xref=byhand, g_yaw=None))
    torch.cuda.synchronize(plan.device)
    worst = tg.worst_ratio(_host(given), _host(spread), S)
    print("g_yaw given against spread by hand, worst / (1e-12 S):", worst)
    assert max(worst.values()) <= 1.0
    none = plan.traj_vjp(*a, **dict(g, g_yaw=None))
    assert not torch.equal(none["x0"], given["x0"])


def test_repeatable_and_position_independent(plan):
    """The batch twice, and once in a permuted order: bitwise-equal rows."""
    N, B = 16, 67
    c, _, _ = _case(N, B)
    a, g, t = _args(plan, c), _grads(plan, c), _tangents(plan, c)
    perm = torch.as_tensor(np.random.default_rng(7).permutation(B)).to(plan.device)
    take = lambda x: x[perm].contiguous()                                    # noqa: E731
    ap = [take(x) for x in a[:5]] + a[5:]                 # (hip is shared, dt a number)
    v1, v2 = plan.traj_vjp(*a, **g), plan.traj_vjp(*a, **g)
    vp = plan.traj_vjp(*ap, **{n: take(x) for n, x in g.items()})
    j1, j2 = plan.traj_jvp(*a, t), plan.traj_jvp(*a, t)
    jp = plan.traj_jvp(*ap, {n: take(x) for n, x in t.items()})
    torch.cuda.synchronize(plan.device)
    for first, again, moved in ((v1, v2, vp), (j1, j2, jp)):
        for n in first:
            assert torch.equal(first[n], again[n]), n
            assert torch.equal(first[n][perm], moved[n]), n


def test_graph_capture(plan):
    """Both entries captured on one stream at B = 64, one after the other, replayed once: bitwise
    the eager results."""
    N, B = plan.params.N, 64
    c = tg.random_case(np.random.default_rng(3), B, N)
    a, g, t = _args(plan, c), _grads(plan, c), _tangents(plan, c)
    f64 = dict(dtype=torch.float64, device=plan.device)
    vout = dict(x0=torch.empty(B, 12, **f64), pos_des=torch.empty(B, 3, **f64),
                cmd=torch.empty(B, 4, **f64), foot_lever=torch.empty(B, 4, 3, **f64))
    jout = dict(xref=torch.empty(B, N, 12, device=plan.device),
                r_feet=torch.empty(B, N, 4, 3, device=plan.device), pos_des=torch.empty(B, 3, **f64))

    def both():
        plan.traj_vjp(*a, **g, out=vout)
        plan.traj_jvp(*a, t, out=jout)

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
    ev, ej = plan.traj_vjp(*a, **g), plan.traj_jvp(*a, t)
    torch.cuda.synchronize(plan.device)
    for n in vout:
        assert torch.equal(vout[n], ev[n]) and bool((vout[n] != -1.0).any()), n
    for n in jout:
        assert torch.equal(jout[n], ej[n]) and bool((jout[n] != -1.0).any()), n


def _tick(plan, B, seed):
    """Tick inputs of B robots on the device: (x0, pos_des, cmd, t_now, gait, foot_lever, hip), dt,
    mass, inertia."""
    from cmpc import synth
    t = synth.make_tick_inputs(B, seed=seed, mixed=True, N=plan.params.N)
    f32, f64 = torch.float32, torch.float64
    dev = lambda k, dt: torch.as_tensor(np.ascontiguousarray(t[k]), dtype=dt).to(plan.device)  # noqa: E731
    ins = [dev("x0", f32), dev("pos_des", f64), dev("cmd", f32), dev("t_now", f64), dev("gait", f64),
           dev("foot_lever", f32), dev("hip", f32)]
    return ins, float(t["dt"]), dev("m", f32), dev("I_world", f32)


def test_fp64_chain(plan):
    """64 robots of config 2: Plan.vjp(want=Ad, Bd, xref) -> Plan.dynamics_vjp -> Plan.traj_vjp
    (g_xref, g_r_feet, g_yaw) stays in float64 and matches ref_vjp of the downloaded gradients
    within 1e-12 x S."""
    from cmpc import synth, to_device_batch
    B, N = 64, plan.params.N
    b = synth.make_config(2, B=B)
    d = to_device_batch(b, plan.device)
    m, I, r, xr = (_dev(plan, np.float32(b[k])) for k in ("m", "I_world", "r_legs", "xref"))
    dt = float(b["dt"])
    Ad, Bd, gd = plan.build_dynamics(m, I, r, xr, dt)
    rest = [d["x0"], d["xref"], d["contact"]]
    w, st, _ = plan.solve(Ad, Bd, gd, *rest)
    assert bool((st > 0).all())
    cw = torch.randn(B, 24 * N, generator=torch.Generator().manual_seed(9)).to(plan.device)
    s64 = plan.vjp(Ad, Bd, gd, *rest, cw, w=w, want=("Ad", "Bd", "xref"))
    dyn = plan.dynamics_vjp(m, I, r, xr, dt, g_Ad=s64["Ad"], g_Bd=s64["Bd"], want=("r_feet", "yaw"))
    ins, tdt, _, _ = _tick(plan, B, seed=2500)
    x0, pos_des, cmd, t_now, gait, _, hip = ins
    got = plan.traj_vjp(x0, pos_des, cmd, t_now, gait, hip, tdt, g_xref=s64["xref"],
                        g_r_feet=dyn["r_feet"], g_yaw=dyn["yaw"])
    torch.cuda.synchronize(plan.device)
    h = lambda x: x.cpu().numpy()                                            # noqa: E731
    vals, S = tg.ref_vjp(h(x0), h(pos_des), h(cmd), h(t_now), h(gait), h(hip), tdt, N,
                         g_xref=h(s64["xref"]), g_r_feet=h(dyn["r_feet"]), g_yaw=h(dyn["yaw"]))
    worst = tg.worst_ratio(_host(got), vals, S)
    print("fp64 chain, worst |dev - ref| / (1e-12 S):", worst)
    assert float(got["cmd"].abs().max()) > 0.0 and max(worst.values()) <= 1.0, worst


def test_autograd_layer(plan):
    """generate_traj -> build_dynamics -> solve -> (w . c).sum().backward() with cmd, x0 and
    foot_lever as leaves: each .grad is the same launches' results through the same casts,
    exactly, x0.grad the sum of the direct and the trajectory paths; one traj_vjp launch for
    exactly the leaves; the caller's pos_des is unmodified; under forward_ad with a tangent on
    cmd the tangents of xref and r_feet are Plan.traj_jvp's."""
    import torch.autograd.forward_ad as fwAD
    from cmpc import autograd
    B, N = 64, plan.params.N
    f32, f64 = torch.float32, torch.float64
    (x0, pos_des, cmd, t_now, gait, fl, hip), dt, m, I = _tick(plan, B, seed=2600)
    pd0 = pos_des.clone()
    pd1 = pos_des.clone()
    xr0, ct0, r0 = plan.generate_traj(x0, pd1, cmd, t_now, gait, fl, hip, dt)
    cw = torch.randn(B, 24 * N, generator=torch.Generator().manual_seed(11)).to(plan.device)
    lx, lc, lf = (t.clone().requires_grad_(True) for t in (x0, cmd, fl))
    asked = []
    tvjp = plan.traj_vjp
    plan.traj_vjp = lambda *a, **k: asked.append(tuple(k["want"])) or tvjp(*a, **k)
    try:
        xref, contact, r, pd_out = autograd.generate_traj(plan, lx, pos_des, lc, t_now, gait, lf, hip, dt)
        assert torch.equal(pos_des, pd0) and torch.equal(pd_out, pd1)
        assert torch.equal(xref, xr0) and torch.equal(contact, ct0) and torch.equal(r, r0)
        assert xref.requires_grad and r.requires_grad and pd_out.requires_grad
        assert not contact.requires_grad
        Ad, Bd, gd = autograd.build_dynamics(plan, m, I, r, xref, dt)
        w, st, _ = autograd.solve(plan, Ad, Bd, gd, lx, xref, contact)
        assert bool((st != -10).all())
        (w * cw).sum().backward()
    finally:
        del plan.traj_vjp
    assert asked == [("x0", "cmd", "foot_lever")]
    # the same launches by hand, through the same casts
    A0, B0, g0 = (t.detach() for t in (Ad, Bd, gd))
    s = plan.vjp(A0, B0, g0, x0, xr0, ct0, cw, w=w.detach(), want=("Ad", "Bd", "x0", "xref"))
    dyn = plan.dynamics_vjp(m, I, r0, xr0, dt, g_Ad=s["Ad"].to(f32).to(f64), g_Bd=s["Bd"].to(f32).to(f64),
                            want=("r_feet", "yaw"))
    spread = torch.zeros_like(xr0)
    spread[:, :, 5] = (dyn["yaw"] / N).to(f32)[:, None]
    g_xref = s["xref"].to(f32) + spread
    exp = plan.traj_vjp(x0, pd0, cmd, t_now, gait, hip, dt, g_xref=g_xref.to(f64),
                        g_r_feet=dyn["r_feet"].to(f32).to(f64), want=("x0", "cmd", "foot_lever"))
    assert lc.grad.dtype == f32 and torch.equal(lc.grad, exp["cmd"].to(f32))
    assert torch.equal(lf.grad, exp["foot_lever"].to(f32))
    assert torch.equal(lx.grad, s["x0"].to(f32) + exp["x0"].to(f32))
    for leaf in (lx, lc, lf):
        assert float(leaf.grad.abs().max()) > 0.0 and bool(torch.isfinite(leaf.grad).all())
    assert float(exp["x0"].abs().max()) > 0.0
    # a loss on the desired position the tick leaves reaches pos_des and x0
    lp = pos_des.clone().requires_grad_(True)
    lx2 = x0.clone().requires_grad_(True)
    out = autograd.generate_traj(plan, lx2, lp, cmd, t_now, gait, fl, hip, dt)
    gp = torch.randn(B, 3, dtype=f64, generator=torch.Generator().manual_seed(12)).to(plan.device)
    (out[3] * gp).sum().backward()
    e2 = plan.traj_vjp(x0, pd0, cmd, t_now, gait, hip, dt, g_pos_des=gp, want=("x0", "pos_des"))
    assert lp.grad.dtype == f64 and torch.equal(lp.grad, e2["pos_des"])
    assert torch.equal(lx2.grad, e2["x0"].to(f32))
    # forward mode
    tan = torch.randn(B, 4, generator=torch.Generator().manual_seed(13)).to(plan.device)
    with fwAD.dual_level():
        o = autograd.generate_traj(plan, x0, pos_des, fwAD.make_dual(cmd, tan), t_now, gait, fl, hip, dt)
        ref = plan.traj_jvp(x0, pd0, cmd, t_now, gait, hip, dt, dict(cmd=tan))
        assert torch.equal(fwAD.unpack_dual(o[0]).tangent, ref["xref"])
        assert torch.equal(fwAD.unpack_dual(o[2]).tangent, ref["r_feet"])
        assert torch.equal(fwAD.unpack_dual(o[3]).tangent, ref["pos_des"])
        assert fwAD.unpack_dual(o[1]).tangent is None
        assert float(ref["xref"].abs().max()) > 0.0 and float(ref["r_feet"].abs().max()) > 0.0
        o2 = autograd.generate_traj(plan, x0, pos_des, cmd, t_now, gait, fl, hip, dt)
        assert fwAD.unpack_dual(o2[0]).tangent is None                # no tangent: nothing moves
    assert torch.equal(pos_des, pd0)
    torch.cuda.synchronize(plan.device)


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
    c = tg.random_case(np.random.default_rng(4), B, N)
    a, g, t = _args(plan, c), _grads(plan, c), _tangents(plan, c)
    ins = dict(zip(IN, a[:6]))
    out = plan.traj_vjp(*a, **g)
    jo = plan.traj_jvp(*a, t)
    cases = (("cmpc_traj_vjp_run", _lib.CTrajVjpIO, "g_x0",
              dict(ins, dt=a[6], g_xref=g["g_xref"], g_x0=out["x0"]), ("g_xref",), ("g_x0",)),
             ("cmpc_traj_jvp_run", _lib.CTrajJvpIO, "d_xref",
              dict(ins, dt=a[6], d_cmd=t["cmd"], d_xref=jo["xref"]), ("d_cmd",), ("d_xref",)))
    for entry, mirror, first, ok, given, outputs in cases:
        assert _raw(plan, entry, mirror, B, **ok)[0] == 0
        assert _raw(plan, entry, mirror, 0, **ok)[0] == 0                    # B == 0 returns
        assert _raw(plan, entry, mirror, 0, **dict(ok, x0=None))[0] == 0
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
    ends = dict(cases[0][3], g_x0=None, g_cmd=out["cmd"])
    rc, msg = _raw(plan, "cmpc_traj_vjp_run", _lib.CTrajVjpIO, B,
                   size=_lib.CTrajVjpIO.g_pos_des.offset, **ends)
    assert rc == -22 and "every output is null" in msg
    # the Python layer
    for dt in (0.0, -0.01, float("nan")):
        with pytest.raises((CmpcError, ValueError)):
            plan.traj_vjp(*a[:6], dt, **g)
        with pytest.raises((CmpcError, ValueError)):
            plan.traj_jvp(*a[:6], dt, t)
    with pytest.raises(ValueError):
        plan.traj_vjp(*a)
    with pytest.raises(ValueError):
        plan.traj_vjp(*a, **g, want=())
    with pytest.raises(ValueError):
        plan.traj_vjp(*a, **g, want=("xref",))
    with pytest.raises(ValueError):
        plan.traj_jvp(*a, {})
    with pytest.raises(ValueError):
        plan.traj_jvp(*a, dict(gait=t["cmd"]))
    with pytest.raises(ValueError):
        plan.traj_jvp(*a, t, want=())
    with pytest.raises(ValueError):
        plan.traj_jvp(*a, t, want=("contact",))
    with pytest.raises((TypeError, ValueError)):
        plan.traj_vjp(*a, g_xref=g["g_xref"].to(torch.float32))
    with pytest.raises((TypeError, ValueError)):
        plan.traj_jvp(*a, dict(cmd=t["cmd"].to(torch.float64)))
    with pytest.raises((TypeError, ValueError)):
        plan.traj_vjp(a[0], a[1].to(torch.float32), *a[2:], **g)
    # B == 0 returns
    e = [x[:0].contiguous() for x in a[:5]] + a[5:]
    r0 = plan.traj_vjp(*e, g_xref=g["g_xref"][:0].contiguous())
    j0 = plan.traj_jvp(*e, dict(cmd=t["cmd"][:0].contiguous()))
    assert r0["x0"].shape == (0, 12) and j0["r_feet"].shape == (0, N, 4, 3)
    torch.cuda.synchronize(plan.device)
