"""GPU: gradients and tangents of the rigid-body plant on the device (cmpc_srb_vjp_run /
cmpc_srb_jvp_run, Plan.srb_vjp / Plan.srb_jvp, cmpc.autograd.srb_step and cmpc.autograd.tick)
against srb_grad_util's complex-step reference of the unmodified oracle.

Inputs are srb_util.make_plant_inputs draws plus one constructed robot whose leg lifts and lands
again within one call; gradients and tangents are standard normal.  Bars: the vjp within 1e-12 x S
per robot and entry (dyn_grad_util.TOL, the project's bar for these kernels; the reference's own
noise is below 1e-14 x S, tests/test_srb_grad.py); the jvp's fp32 outputs within one fp32 rounding
2^-23 |ref| plus 1e-12 x S; an entry whose S is 0 exactly 0.  Shapes: B = 1, 63, 64, 65 and 257
around the 64-robot block, nsub = 1, 7, 8, 9 and 20 around the tape's segment of 8 substeps, 24 and
25 on either side of the threshold between the vjp kernel's two tape sizes, 64 the longest call,
B = 8197 bitwise against B = 67.

Measured on an MI355X, worst ratio to the bar over all cases: vjp 0.039
(g_inertia_body at nsub = 7; x, feet, force and mass stay below 4e-3), the jvp's fp32 outputs 0.496,
which is the half-ulp of their one rounding against a bar of one ulp (0.992 of the half-ulp bar
below), the adjoint identity between the entries 0.27, again the fp32 rounding of d_x_out
and d_feet_out, which the bar counts at one ulp per entry and no cancellation."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import srb_grad_util as sg

pytestmark = pytest.mark.gpu

IN = ("t_now", "gait", "mass", "inertia_body", "force", "hip", "x", "feet", "contact_state")
DTYPES = dict(t_now=np.float64, gait=np.float64, mass=np.float32, inertia_body=np.float32,
              force=np.float32, hip=np.float32, x=np.float32, feet=np.float32,
              contact_state=np.uint8)


@functools.lru_cache(maxsize=None)
def _case(B, seed, nsub):
    """The case with both references, computed once and shared (not modified)."""
    inp, g, d = sg.case(B, seed, nsub)
    J = sg.jacobian(inp, sg.H, nsub)
    return inp, g, d, sg.ref_vjp(J, g), sg.ref_jvp(J, d)


def _dev(plan, a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype)).to(plan.device)


def _args(plan, inp, nsub):
    return [_dev(plan, inp[k], DTYPES[k]) for k in IN] + [nsub, sg.H]


def _grads(plan, g):
    return dict(g_x=_dev(plan, g[:, :12]), g_feet=_dev(plan, g[:, 12:].reshape(-1, 4, 3)))


def _tangents(plan, d):
    return {n: _dev(plan, t, np.float32) for n, t in sg.split(d).items()}


def _host(res):
    return {n: t.cpu().numpy() for n, t in res.items()}


@pytest.mark.parametrize("B,seed,nsub", sg.CASES)
def test_against_reference(plan, B, seed, nsub):
    inp, g, d, (vv, vS), (jv, jS) = _case(B, seed, nsub)
    a = _args(plan, inp, nsub)
    before = [t.clone() for t in a[:9]]
    rv = plan.srb_vjp(*a, **_grads(plan, g))
    rj = plan.srb_jvp(*a, _tangents(plan, d))
    torch.cuda.synchronize(plan.device)
    assert all(torch.equal(t, b) for t, b in zip(a[:9], before))            # inputs unmodified
    gv, gj = _host(rv), _host(rj)
    assert tuple(gv) == sg.INPUTS and tuple(gj) == sg.OUTPUTS
    assert all(gv[n].dtype == np.float64 and gv[n].shape == vv[n].shape for n in gv)
    assert all(gj[n].dtype == np.float32 and gj[n].shape == jv[n].shape for n in gj)
    wv = sg.worst_ratio(gv, vv, vS)
    wj = sg.worst_ratio(gj, jv, jS, rel=sg.REL32)
    print(f"B={B} seed={seed} nsub={nsub} worst |dev - ref| / (1e-12 S): vjp", wv,
          " / (2^-23 |ref| + 1e-12 S): jvp", wj)
    assert max(wv.values()) <= 1.0, wv
    assert max(wj.values()) <= 1.0, wj
    # the fp64 arithmetic behind the fp32 outputs: a value within 1e-12 S of the reference, rounded
    # once, is within half an ulp of it plus 1e-12 S
    wh = sg.worst_ratio(gj, jv, jS, rel=sg.REL32 / 2)
    print("    jvp / (2^-24 |ref| + 1e-12 S):", wh)
    assert max(wh.values()) <= 1.0, wh
    # the exact zeros: force of a leg in swing throughout, feet of a leg not in stance before it
    # lands, the height of a landed foot's tangent
    st = sg.schedule(inp, sg.H, nsub)
    swing = ~st[:, 1:].any(1)
    assert np.all(gv["force"].reshape(-1, 4, 3)[swing] == 0.0)
    assert np.all(vS["force"].reshape(-1, 4, 3)[swing] == 0.0)
    landed = (st[:, 1:] & ~st[:, :-1]).any(1)
    assert np.all(gj["feet"][landed][:, 2] == 0.0)
    assert np.all(vS["x"] > 0.0) and np.all(jS["x"] > 0.0)
    if B > 1 and nsub == 20:
        assert swing.any() and landed.any() and np.abs(gj["feet"]).max() > 0.0


def test_grid_and_block_tails(plan):
    """The main case tiled to B = 8197 (129 blocks, the last with 5 robots): every row bitwise
    the B = 67 run's."""
    B, seed, nsub = sg.MAIN
    inp, g, d, _, _ = _case(B, seed, nsub)
    a, gr, ta = _args(plan, inp, nsub), _grads(plan, g), _tangents(plan, d)
    idx = torch.arange(8197, device=plan.device) % B
    take = lambda t: t[idx].contiguous()                                     # noqa: E731
    big = [take(t) for t in a[:5]] + [a[5]] + [take(t) for t in a[6:9]] + a[9:]
    v, j = plan.srb_vjp(*a, **gr), plan.srb_jvp(*a, ta)
    vb = plan.srb_vjp(*big, **{n: take(t) for n, t in gr.items()})
    jb = plan.srb_jvp(*big, {n: take(t) for n, t in ta.items()})
    torch.cuda.synchronize(plan.device)
    for small, tiled in ((v, vb), (j, jb)):
        for n in small:
            assert tiled[n].shape[0] == 8197 and torch.equal(small[n][idx], tiled[n]), n


def test_adjoint_identity_between_the_entries(plan):
    """<g, d_out> with the device's tangents against <g_in, d> with the device's gradients, per
    robot.  The bar is what the reference test allows each entry: 2^-23 sum |g_i| |dout_i| for the
    rounding of the fp32 outputs, plus 1e-12 x (sum |g_i| S_i on the left, sum S_i |d_i| on the
    right)."""
    B, seed, nsub = sg.MAIN
    inp, g, d, (_, vS), (_, jS) = _case(B, seed, nsub)
    a = _args(plan, inp, nsub)
    gv = _host(plan.srb_vjp(*a, **_grads(plan, g)))
    gj = _host(plan.srb_jvp(*a, _tangents(plan, d)))
    torch.cuda.synchronize(plan.device)
    rows = lambda x: np.asarray(x, np.float64).reshape(B, -1)                # noqa: E731
    dout = np.concatenate([rows(gj[n]) for n in sg.OUTPUTS], 1)
    gin = np.concatenate([rows(gv[n]) for n in sg.INPUTS], 1)
    Sj = np.concatenate([rows(jS[n]) for n in sg.OUTPUTS], 1)
    Sv = np.concatenate([rows(vS[n]) for n in sg.INPUTS], 1)
    left, right = (g * dout).sum(1), (gin * d).sum(1)
    bar = (sg.REL32 * (np.abs(g) * np.abs(dout)).sum(1) +
           sg.TOL * ((np.abs(g) * Sj).sum(1) + (Sv * np.abs(d)).sum(1)))
    ratio = np.abs(left - right) / bar
    print("worst adjoint mismatch / bar:", float(ratio.max()))
    assert np.all(np.abs(left) > 0.0) and ratio.max() <= 1.0


def test_subsets_and_null_inputs(plan):
    """An output asked for alone is bitwise the one asked for with all the others; a NULL
    gradient or tangent gives the values of an array of zeros (==: the sign of a zero may
    differ)."""
    B, seed, nsub = sg.MAIN
    inp, g, d, _, _ = _case(B, seed, nsub)
    a, gr, ta = _args(plan, inp, nsub), _grads(plan, g), _tangents(plan, d)
    every = plan.srb_vjp(*a, **gr)
    for n in sg.INPUTS:
        alone = plan.srb_vjp(*a, **gr, want=(n,))
        assert set(alone) == {n} and torch.equal(alone[n], every[n]), n
    pair = plan.srb_vjp(*a, **gr, want=("x", "force"))       # (neither mass nor inertia: skipped)
    assert torch.equal(pair["x"], every["x"]) and torch.equal(pair["force"], every["force"])
    allj = plan.srb_jvp(*a, ta)
    for n in sg.OUTPUTS:
        alone = plan.srb_jvp(*a, ta, want=(n,))
        assert set(alone) == {n} and torch.equal(alone[n], allj[n]), n
    for n in gr:
        null = plan.srb_vjp(*a, **dict(gr, **{n: None}))
        zero = plan.srb_vjp(*a, **dict(gr, **{n: torch.zeros_like(gr[n])}))
        for o in sg.INPUTS:
            assert bool((null[o] == zero[o]).all()), (n, o)
        assert any(not torch.equal(null[o], every[o]) for o in sg.INPUTS), n
    for n in ta:
        null = plan.srb_jvp(*a, {k: v for k, v in ta.items() if k != n})
        zero = plan.srb_jvp(*a, dict(ta, **{n: torch.zeros_like(ta[n])}))
        for o in sg.OUTPUTS:
            assert bool((null[o] == zero[o]).all()), (n, o)
        assert any(not torch.equal(null[o], allj[o]) for o in sg.OUTPUTS), n
    torch.cuda.synchronize(plan.device)


def test_repeatable_position_independent_and_strided_force(plan):
    """The batch twice, once in a permuted order, and once with the forces read off the rows of a
    solution w (row stride 24 N): bitwise-equal rows."""
    B, seed, nsub = sg.MAIN
    inp, g, d, _, _ = _case(B, seed, nsub)
    a, gr, ta = _args(plan, inp, nsub), _grads(plan, g), _tangents(plan, d)
    perm = torch.as_tensor(np.random.default_rng(7).permutation(B)).to(plan.device)
    take = lambda t: t[perm].contiguous()                                    # noqa: E731
    ap = [take(t) for t in a[:5]] + [a[5]] + [take(t) for t in a[6:9]] + a[9:]
    N = plan.params.N
    w = torch.randn(B, 24 * N, generator=torch.Generator().manual_seed(5)).to(plan.device)
    w[:, 12 * N:12 * N + 12] = a[4]
    aw = a[:4] + [w[:, 12 * N:]] + a[5:]
    assert aw[4].stride(0) == 24 * N and aw[4].shape[1] == 12 * N
    v1, v2 = plan.srb_vjp(*a, **gr), plan.srb_vjp(*a, **gr)
    vp, vw = plan.srb_vjp(*ap, **{n: take(t) for n, t in gr.items()}), plan.srb_vjp(*aw, **gr)
    j1, j2 = plan.srb_jvp(*a, ta), plan.srb_jvp(*a, ta)
    jp, jw = plan.srb_jvp(*ap, {n: take(t) for n, t in ta.items()}), plan.srb_jvp(*aw, ta)
    torch.cuda.synchronize(plan.device)
    for first, again, moved, strided in ((v1, v2, vp, vw), (j1, j2, jp, jw)):
        for n in first:
            assert torch.equal(first[n], again[n]), n
            assert torch.equal(first[n][perm], moved[n]), n
            assert torch.equal(first[n], strided[n]), n
    assert vw["force"].shape == (B, 12)


def test_graph_capture(plan):
    """Both entries captured on one stream at B = 64, one after the other, replayed once: bitwise
    the eager results."""
    B, seed, nsub = 64, 164, 20
    inp, g, d, _, _ = _case(B, seed, nsub)
    a, gr, ta = _args(plan, inp, nsub), _grads(plan, g), _tangents(plan, d)
    f64 = dict(dtype=torch.float64, device=plan.device)
    vout = dict(x=torch.empty(B, 12, **f64), feet=torch.empty(B, 4, 3, **f64),
                force=torch.empty(B, 12, **f64), mass=torch.empty(B, **f64),
                inertia_body=torch.empty(B, 3, 3, **f64))
    jout = dict(x=torch.empty(B, 12, device=plan.device), feet=torch.empty(B, 4, 3, device=plan.device))

    def both():
        plan.srb_vjp(*a, **gr, out=vout)
        plan.srb_jvp(*a, ta, out=jout)

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
    ev, ej = plan.srb_vjp(*a, **gr), plan.srb_jvp(*a, ta)
    torch.cuda.synchronize(plan.device)
    for n in vout:
        assert torch.equal(vout[n], ev[n]) and bool((vout[n] != -1.0).any()), n
    for n in jout:
        assert torch.equal(jout[n], ej[n]) and bool((jout[n] != -1.0).any()), n


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
    B, nsub = 3, 20
    inp, g, d = sg.case(3, 4, nsub)
    a, gr, ta = _args(plan, inp, nsub), _grads(plan, g), _tangents(plan, d)
    ins = dict(zip(IN, a[:9]), force_stride=12, nsub=nsub, dt=sg.H)
    out = plan.srb_vjp(*a, **gr)
    jo = plan.srb_jvp(*a, ta)
    cases = (("cmpc_srb_vjp_run", _lib.CSrbVjpIO, "g_x",
              dict(ins, g_x_out=gr["g_x"], g_x=out["x"]), ("g_x_out",), ("g_x",)),
             ("cmpc_srb_jvp_run", _lib.CSrbJvpIO, "d_x_out",
              dict(ins, d_force=ta["force"], d_x_out=jo["x"]), ("d_force",), ("d_x_out",)))
    for entry, mirror, first, ok, given, outputs in cases:
        assert _raw(plan, entry, mirror, B, **ok)[0] == 0
        assert _raw(plan, entry, mirror, 0, **ok)[0] == 0                    # B == 0 returns
        assert _raw(plan, entry, mirror, 0, **dict(ok, x=None))[0] == 0
        bad = [dict(handle=False), dict(B=-1), dict(size=getattr(mirror, first).offset), dict(size=4)]
        bad += [dict(nsub=v) for v in (0, -1, 65)]
        bad += [dict(dt=v) for v in (0.0, -0.01, float("nan"), float("inf"))]
        bad += [dict(force_stride=11)]
        bad += [{n: None} for n in IN]
        bad += [{n: None for n in given}, {n: None for n in outputs}]
        for change in bad:
            kw = dict(ok, **{k: v for k, v in change.items() if k not in ("handle", "B", "size")})
            rc, msg = _raw(plan, entry, mirror, change.get("B", B), size=change.get("size"),
                           handle=change.get("handle", True), **kw)
            assert rc == -22 and entry in msg, (entry, change, rc, msg)
        assert _raw(plan, entry, mirror, B, **dict(ok, nsub=64))[0] == 0     # the longest call
    # a struct that ends after the first output reads the outputs past it as NULL
    ends = dict(cases[0][3], g_x=None, g_force=out["force"])
    rc, msg = _raw(plan, "cmpc_srb_vjp_run", _lib.CSrbVjpIO, B,
                   size=_lib.CSrbVjpIO.g_feet.offset, **ends)
    assert rc == -22 and "every output is null" in msg
    # the Python layer
    for dt in (0.0, -0.01, float("nan")):
        with pytest.raises((CmpcError, ValueError)):
            plan.srb_vjp(*a[:10], dt, **gr)
        with pytest.raises((CmpcError, ValueError)):
            plan.srb_jvp(*a[:10], dt, ta)
    for n in (0, 65):
        with pytest.raises((CmpcError, ValueError)):
            plan.srb_vjp(*a[:9], n, sg.H, **gr)
        with pytest.raises((CmpcError, ValueError)):
            plan.srb_jvp(*a[:9], n, sg.H, ta)
    with pytest.raises(ValueError):
        plan.srb_vjp(*a)
    with pytest.raises(ValueError):
        plan.srb_vjp(*a, **gr, want=())
    with pytest.raises(ValueError):
        plan.srb_vjp(*a, **gr, want=("gait",))
    with pytest.raises(ValueError):
        plan.srb_jvp(*a, {})
    with pytest.raises(ValueError):
        plan.srb_jvp(*a, dict(gait=ta["x"]))
    with pytest.raises(ValueError):
        plan.srb_jvp(*a, ta, want=())
    with pytest.raises(ValueError):
        plan.srb_jvp(*a, ta, want=("force",))
    with pytest.raises((TypeError, ValueError)):
        plan.srb_vjp(*a, g_x=gr["g_x"].to(torch.float32))
    with pytest.raises((TypeError, ValueError)):
        plan.srb_jvp(*a, dict(x=ta["x"].to(torch.float64)))
    with pytest.raises((TypeError, ValueError)):
        plan.srb_vjp(*a[:6], a[6].to(torch.float64), *a[7:], **gr)
    with pytest.raises(ValueError):
        plan.srb_vjp(*a[:4], a[4][:, :11], *a[5:], **gr)                     # force too narrow
    # B == 0 returns
    e = [t[:0].contiguous() for t in a[:5]] + [a[5]] + [t[:0].contiguous() for t in a[6:9]] + a[9:]
    r0 = plan.srb_vjp(*e, g_x=gr["g_x"][:0].contiguous())
    j0 = plan.srb_jvp(*e, dict(x=ta["x"][:0].contiguous()))
    assert r0["inertia_body"].shape == (0, 3, 3) and j0["feet"].shape == (0, 4, 3)
    torch.cuda.synchronize(plan.device)


def test_autograd_srb_step(plan):
    """autograd.srb_step: .grad of x, feet, force (a slice of a leaf w), mass and inertia is one
    hand Plan.srb_vjp launch through the same casts, exactly; one launch for exactly the leaves;
    forward-mode tangents are Plan.srb_jvp's; the caller's tensors are unmodified and x', feet',
    contact' are an in-place Plan.srb_step on clones, bitwise."""
    import torch.autograd.forward_ad as fwAD
    from cmpc import autograd
    B, seed, nsub = sg.MAIN
    inp, g, d, _, _ = _case(B, seed, nsub)
    a, gr, ta = _args(plan, inp, nsub), _grads(plan, g), _tangents(plan, d)
    t_now, gait, mass, Ib, force, hip, x, feet, cs = a[:9]
    f32, f64 = torch.float32, torch.float64
    N = plan.params.N
    w = torch.randn(B, 24 * N, generator=torch.Generator().manual_seed(6)).to(plan.device)
    w[:, 12 * N:12 * N + 12] = force
    before = [t.clone() for t in (x, feet, cs)]
    x1, f1, c1 = (t.clone() for t in (x, feet, cs))
    plan.srb_step(t_now, gait, mass, Ib, force, hip, x1, f1, c1, nsub, sg.H)
    lx, lf, lw, lm, lI = (t.clone().requires_grad_(True) for t in (x, feet, w, mass, Ib))
    asked = []
    svjp = plan.srb_vjp
    plan.srb_vjp = lambda *p, **k: asked.append(tuple(k["want"])) or svjp(*p, **k)
    try:
        xo, fo, co = autograd.srb_step(plan, t_now, gait, lm, lI, lw[:, 12 * N:12 * N + 12], hip, lx,
                                       lf, cs, nsub, sg.H)
        assert torch.equal(xo, x1) and torch.equal(fo, f1) and torch.equal(co, c1)
        assert xo.requires_grad and fo.requires_grad and not co.requires_grad
        ((xo * gr["g_x"].to(f32)).sum() + (fo * gr["g_feet"].to(f32)).sum()).backward()
        # x alone
        lx2 = x.clone().requires_grad_(True)
        xo2, _, _ = autograd.srb_step(plan, t_now, gait, mass, Ib, force, hip, lx2, feet, cs, nsub, sg.H)
        (xo2 * gr["g_x"].to(f32)).sum().backward()
    finally:
        del plan.srb_vjp
    assert asked == [sg.INPUTS, ("x",)]
    assert all(torch.equal(t, b) for t, b in zip((x, feet, cs), before))
    exp = plan.srb_vjp(*a, g_x=gr["g_x"].to(f32).to(f64), g_feet=gr["g_feet"].to(f32).to(f64))
    assert lx.grad.dtype == f32 and torch.equal(lx.grad, exp["x"].to(f32))
    assert torch.equal(lf.grad, exp["feet"].to(f32)) and torch.equal(lm.grad, exp["mass"].to(f32))
    assert torch.equal(lI.grad, exp["inertia_body"].to(f32))
    gw = torch.zeros_like(w)
    gw[:, 12 * N:12 * N + 12] = exp["force"].to(f32)
    assert torch.equal(lw.grad, gw) and float(lw.grad.abs().max()) > 0.0
    e2 = plan.srb_vjp(*a, g_x=gr["g_x"].to(f32).to(f64), want=("x",))
    assert torch.equal(lx2.grad, e2["x"].to(f32))
    # forward mode
    with fwAD.dual_level():
        o = autograd.srb_step(plan, t_now, gait, mass, Ib, fwAD.make_dual(force, ta["force"]), hip,
                              fwAD.make_dual(x, ta["x"]), feet, cs, nsub, sg.H)
        ref = plan.srb_jvp(*a, dict(x=ta["x"], force=ta["force"]))
        assert torch.equal(fwAD.unpack_dual(o[0]).tangent, ref["x"])
        assert torch.equal(fwAD.unpack_dual(o[1]).tangent, ref["feet"])
        assert fwAD.unpack_dual(o[2]).tangent is None
        assert float(ref["x"].abs().max()) > 0.0
        o2 = autograd.srb_step(plan, t_now, gait, mass, Ib, force, hip, x, feet, cs, nsub, sg.H)
        assert fwAD.unpack_dual(o2[0]).tangent is None                # no tangent: nothing moves
    torch.cuda.synchronize(plan.device)


def _tick_inputs(plan, B, seed):
    """Synthetic tick inputs of B robots on the device: the state dict and cmd, gait, hip, mass,
    inertia_body, dt."""
    from cmpc import synth
    from oracle import srb_ref
    import srb_util
    t = synth.make_tick_inputs(B, seed=seed, mixed=True, N=plan.params.N)
    f32, f64 = np.float32, np.float64
    feet = srb_util.f32(t["foot_lever"] + t["x0"][:, None, 0:3])
    g = t["gait"]
    cs = srb_util.mask_bits(srb_ref.stance_mask(t["t_now"], g[:, 0], g[:, 1], g[:, 2:6]))
    state = dict(x=_dev(plan, t["x0"], f32), feet=_dev(plan, feet, f32),
                 contact_state=_dev(plan, cs, np.uint8), pos_des=_dev(plan, t["pos_des"], f64),
                 t=_dev(plan, t["t_now"], f64))
    Ib = np.broadcast_to(synth.INERTIA_BODY, (B, 3, 3))
    return (state, _dev(plan, t["cmd"], f32), _dev(plan, g, f64), _dev(plan, t["hip"], f32),
            _dev(plan, t["m"], f32), _dev(plan, Ib, f32), float(t["dt"]))


def test_tick_and_rollout(plan):
    """One autograd.tick: the forward values are the hand-chained Plan calls', bitwise, and
    cmd.grad and x.grad the hand-chained vjp -> dynamics_vjp -> traj_vjp plus srb_vjp launches'
    through the same casts, exactly.  Three ticks with the loss (x_3 . c).sum() and the leaves cmd
    of tick 0 and x_0: finite, nonzero gradients, and <c, dx_3> from forward_ad with tangents on
    both leaves against <grad, d> from backward -- a wiring check across the whole chain in both
    modes with every cast.  The two sides pass through different fp32 roundings and the closed
    loop cancels, so no bar can be derived: a missing path or a wrong sign gives O(1), and the
    relative mismatch against sum |terms| is asserted <= 1e-3.

    Measured on an MI355X: x.grad of one tick equals the hand chain bit for bit (max |x.grad| 44);
the three-tick mismatch is 6.7e-7 of sum |terms|, the size of the fp32 casts between the layers."""
    import torch.autograd.forward_ad as fwAD
    from cmpc import autograd
    from cmpc.closed_loop import rot_zyx
    B, N, nsub = 64, plan.params.N, 20
    f32, f64 = torch.float32, torch.float64
    state, cmd, gait, hip, mass, Ib, dt = _tick_inputs(plan, B, seed=2700)
    keep = {k: v.clone() for k, v in state.items()}
    gen = torch.Generator().manual_seed(21)
    c = torch.randn(B, 12, generator=gen).to(plan.device)
    # one tick by hand
    x, feet = state["x"], state["feet"]
    lever = feet - x[:, None, 0:3]
    Rm = rot_zyx(x[:, 3:6])
    RI = (Rm[:, :, :, None] * Ib[:, None, :, :]).sum(2)
    Iw = (RI[:, :, None, :] * Rm[:, None, :, :]).sum(3)
    pd1 = state["pos_des"].clone()
    xr, ct, rf = plan.generate_traj(x, pd1, cmd, state["t"], gait, lever, hip, dt)
    Ad, Bd, gd = plan.build_dynamics(mass, Iw, rf, xr, dt)
    w0, st0, _ = plan.solve(Ad, Bd, gd, x, xr, ct)
    x1, f1, c1 = x.clone(), feet.clone(), state["contact_state"].clone()
    plan.srb_step(state["t"], gait, mass, Ib, w0[:, 12 * N:], hip, x1, f1, c1, nsub, dt / nsub)
    assert bool((st0 > 0).all())
    lc, lx = cmd.clone().requires_grad_(True), x.clone().requires_grad_(True)
    s1, w, st = autograd.tick(plan, dict(state, x=lx), lc, gait, hip, mass, Ib, dt, nsub)
    assert torch.equal(w, w0) and torch.equal(st, st0)
    assert torch.equal(s1["x"], x1) and torch.equal(s1["feet"], f1)
    assert torch.equal(s1["contact_state"], c1) and torch.equal(s1["pos_des"], pd1)
    assert torch.equal(s1["t"], state["t"] + dt)
    assert all(torch.equal(state[k], keep[k]) for k in state)
    (s1["x"] * c).sum().backward()
    # the same launches by hand: the plant, then the solve, the dynamics and the trajectory
    pre = (state["t"], gait, mass, Ib, w0[:, 12 * N:], hip, x, feet, state["contact_state"])
    sv = plan.srb_vjp(*pre, nsub, dt / nsub, g_x=c.to(f64), want=("x", "feet", "force"))
    gw = torch.zeros_like(w0)
    gw[:, 12 * N:12 * N + 12] = sv["force"].to(f32)
    s = plan.vjp(Ad, Bd, gd, x, xr, ct, gw, w=w0, want=("Ad", "Bd", "x0", "xref"))
    dyn = plan.dynamics_vjp(mass, Iw, rf, xr, dt, g_Ad=s["Ad"].to(f32).to(f64),
                            g_Bd=s["Bd"].to(f32).to(f64), want=("inertia", "r_feet", "yaw"))
    spread = torch.zeros_like(xr)
    spread[:, :, 5] = (dyn["yaw"] / N).to(f32)[:, None]
    tr = plan.traj_vjp(x, state["pos_des"], cmd, state["t"], gait, hip, dt,
                       g_xref=(s["xref"].to(f32) + spread).to(f64),
                       g_r_feet=dyn["r_feet"].to(f32).to(f64), want=("x0", "cmd", "foot_lever"))
    assert torch.equal(lc.grad, tr["cmd"].to(f32)) and float(lc.grad.abs().max()) > 0.0
    # x: the plant, the solve, the trajectory, the lever feet - p, and R(rpy) I_body R' (by torch)
    lx2 = x.clone().requires_grad_(True)
    R2 = rot_zyx(lx2[:, 3:6])
    RI2 = (R2[:, :, :, None] * Ib[:, None, :, :]).sum(2)
    Iw2 = (RI2[:, :, None, :] * R2[:, None, :, :]).sum(3)
    lev2 = feet - lx2[:, None, 0:3]
    ((Iw2 * dyn["inertia"].to(f32)).sum() + (lev2 * tr["foot_lever"].to(f32)).sum()).backward()
    # (summed in the order the backward pass meets them: plant, solve, trajectory, then the torch
    # ops, whose two parts fall on different columns)
    expect = ((sv["x"].to(f32) + s["x0"].to(f32)) + tr["x0"].to(f32)) + lx2.grad
    print("one tick: max |x.grad - hand chain|:", float((lx.grad - expect).abs().max()),
          " of", float(lx.grad.abs().max()))
    assert torch.equal(lx.grad, expect) and float(lx.grad.abs().max()) > 0.0

    # three ticks
    def rollout(cmd0, x0):
        stt = dict(state, x=x0)
        for k in range(3):
            stt, _, status = autograd.tick(plan, stt, cmd0 if k == 0 else cmd, gait, hip, mass, Ib,
                                           dt, nsub)
            assert bool((status > 0).all()), k
        return stt["x"]

    lc, lx = cmd.clone().requires_grad_(True), x.clone().requires_grad_(True)
    (rollout(lc, lx) * c).sum().backward()
    for leaf in (lc, lx):
        assert bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0.0
    dc = torch.randn(B, 4, generator=gen).to(plan.device)
    dx = torch.randn(B, 12, generator=gen).to(plan.device)
    with fwAD.dual_level():
        x3 = rollout(fwAD.make_dual(cmd, dc), fwAD.make_dual(x, dx))
        tan = fwAD.unpack_dual(x3).tangent
    fwd = (c * tan).to(f64).sum(1)
    terms = torch.cat([(lc.grad * dc).to(f64), (lx.grad * dx).to(f64)], 1)
    bwd = terms.sum(1)
    scale = terms.abs().sum(1) + (c * tan).to(f64).abs().sum(1)
    mismatch = float(((fwd - bwd).abs() / scale).max())
    print("three ticks: worst |<c, dx_3> - <grad, d>| / sum |terms|:", mismatch)
    assert mismatch <= 1e-3
    torch.cuda.synchronize(plan.device)
