"""GPU: forward-mode derivatives of a solved batch (cmpc_jvp_run / Plan.jvp / cmpc.autograd,
include/cmpc.h) against the two float64 NumPy references of tests/jvp_util.py on the same
fp32-rounded arrays.

Bar (jvp_util): |dev - ref| <= 1e-8 x S (vjp_util.TOL_REL), S = max|du_ref| of the instance for
the forces and the absolute-value rollout for the states; where S is 0 the device value must be
exactly 0, as it must on every entry of jvp_util.zero_rule.  Every instance is held to it against
reference (b), the kernel's route in NumPy, and a subset against (a), the dense KKT solve with
the differenced assembly, which test_jvp.py ties to (b) within 1e-9 x S and to central
differences.

Measured on an MI355X: on the five fixture sets the worst ratio to the bar is 4.2e-4 against (a)
(forces, qp_weights_A) and 3.4e-5 against (b); on the arbitrary masks 4.2e-2 against (a) (forces,
N = 16, instance 1) and 1.9e-5 against (b).  No instance is near the bar."""
import ctypes

import numpy as np
import pytest
import torch

import gain_util
import jvp_util
import kkt_util
import vjp_util
from test_gpu_gain import random_case, _fixture, _dev

pytestmark = pytest.mark.gpu
IN = ("Ad", "Bd", "gd", "x0", "xref", "contact")
ALL = jvp_util.TANGENTS
_tan = {}


def _theta(case, params):
    """The batched inputs a tangent can belong to, the plan's constants repeated where the case
    has no rows of its own."""
    B = len(case["Ad"])
    iv = [kkt_util.instance_values(case, i, params) for i in range(B)]
    t = {k: case[k] for k in ("Ad", "Bd", "gd", "x0", "xref")}
    t.update({k: np.stack([v[k] for v in iv]) for k in ("Q", "R")})
    t.update({k: np.array([v[k] for v in iv]) for k in ("mu", "fz_min")})
    return t


def _jvp(plan, case, tan, idx=None, use_w=True, faces=None):
    """Plan.jvp on (the instances idx of) a case -> (B, 24N) numpy array."""
    sel = (lambda a: a) if idx is None else (lambda a: a[idx])
    kw = {k: _dev(plan, sel(case[k])) for k in ("mu", "fz_min", "Q", "R") if k in case}
    out = plan.jvp(*[_dev(plan, sel(case[k])) for k in IN],
                   {n: _dev(plan, sel(v)) for n, v in tan.items()},
                   w=_dev(plan, sel(case["w"])) if use_w else None,
                   faces=None if faces is None else _dev(plan, sel(faces)), **kw)
    torch.cuda.synchronize(plan.device)
    B, N = len(sel(case["Ad"])), case["Bd"].shape[1]
    assert tuple(out.shape) == (B, 24 * N) and out.dtype == torch.float64
    return out.cpu().numpy()


def _fixture_tan(plan, name, tag):
    case, faces = _fixture(plan, name, tag)
    if (name, tag) not in _tan:
        _tan[(name, tag)] = jvp_util.random_tangents(np.random.default_rng(17),
                                                     _theta(case, plan.params))
    return case, faces, _tan[(name, tag)]


def _refs(case, faces, tan, params, i, dense=False):
    """-> (reference (b), S_x, S_u, reference (a) or None) of instance i."""
    iv = kkt_util.instance_values(case, i, params)
    args, kw = gain_util.instance_args(case, i, iv)
    t = {n: v[i] for n, v in tan.items()}
    b, info = jvp_util.ref_riccati(*args, faces[i], tangents=t, **kw)
    a = jvp_util.ref_dense(*args, faces[i], tangents=t, **kw) if dense else None
    return (b,) + jvp_util.scales(args[0], args[1], b, info) + (a,)


def _check(dev, case, faces, tan, params, rows, dense_rows, what):
    """Instances `rows` of dev against reference (b), `dense_rows` also against (a), and the zero
    rule; prints the worst ratio (states, forces) per reference before asserting."""
    worst = {"a": [0.0, 0.0], "b": [0.0, 0.0]}
    at = {"a": [-1, -1], "b": [-1, -1]}
    N = case["Bd"].shape[1]
    for i in rows:
        assert np.all(np.isfinite(dev[i])), (what, i)
        zero = jvp_util.zero_rule(case["contact"][i], faces[i]).ravel()
        assert np.all(dev[i][12 * N:][zero] == 0.0), (what, i)
        b, S_x, S_u, a = _refs(case, faces, tan, params, i, i in dense_rows)
        for tag, ref in (("b", b), ("a", a)):
            if ref is not None:
                for j, r in enumerate(jvp_util.worst_ratio(dev[i], ref, S_x, S_u, vjp_util.TOL_REL)):
                    if r > worst[tag][j]:
                        worst[tag][j], at[tag][j] = r, i
    print(what, "worst |dev - ref| / (1e-8 S) (states, forces): dense KKT (a)", worst["a"],
          "at", at["a"], "riccati (b)", worst["b"], "at", at["b"])
    assert max(worst["a"]) <= 1.0 and max(worst["b"]) <= 1.0, (what, worst, at)


@pytest.mark.parametrize("name,tag", kkt_util.FIXTURES)
def test_fixtures_faces_from_w(plan, name, tag):
    """The five fixture sets with their per-instance mu / fz_min / Q / R, faces read off w, all
    nine tangents random; (b) on every instance, (a) on every fourth."""
    case, faces, tan = _fixture_tan(plan, name, tag)
    dev = _jvp(plan, case, tan)
    B = len(faces)
    _check(dev, case, faces, tan, plan.params, range(B), set(range(0, B, 4)), f"{name}{tag}")
    # the faces given back are bitwise the same
    assert np.array_equal(_jvp(plan, case, tan, use_w=False, faces=faces), dev)


def test_single_tangents_and_their_sum(plan):
    """Each tangent alone against (b) on every eighth instance of qp_weights _A, and the nine
    results added up against the all-nine result: the map is linear, so they differ by at most
    the bars of the ten results, 1e-8 x (S + sum_i S_i)."""
    case, faces, tan = _fixture_tan(plan, "qp_weights.npz", "_A")
    rows = range(0, len(faces), 8)
    N = plan.params.N
    dev_all = _jvp(plan, case, tan, use_w=False, faces=faces)
    total = np.zeros_like(dev_all)
    S = {i: np.array(_refs(case, faces, tan, plan.params, i)[1:3]) for i in rows}
    for n in ALL:
        one = {n: tan[n]}
        dev = _jvp(plan, case, one, use_w=False, faces=faces)
        _check(dev, case, faces, one, plan.params, rows, set(), f"d_{n} alone")
        total += dev
        for i in rows:
            S[i] = S[i] + np.array(_refs(case, faces, one, plan.params, i)[1:3])
    worst = 0.0
    for i in rows:
        err = np.abs(total[i] - dev_all[i])
        worst = max(worst, err[:12 * N].max() / (vjp_util.TOL_REL * S[i][0]),
                    err[12 * N:].max() / (vjp_util.TOL_REL * S[i][1]))
    print("worst |sum of the nine - all nine| / (1e-8 (S + sum S_i)):", worst)
    assert worst <= 1.0


def test_null_tangent_equals_zero_tangent(plan):
    """A tangent left out and the same tangent as an array of zeros: equal results, also across
    the paths that skip the costates and the primal."""
    case, faces, tan = _fixture_tan(plan, "qp_terrain.npz", "_B")
    zeros = {n: np.zeros_like(v) for n, v in tan.items()}
    for n in ALL:
        rest = {m: v for m, v in tan.items() if m != n}
        assert np.array_equal(_jvp(plan, case, rest), _jvp(plan, case, dict(rest, **{n: zeros[n]}))), n
    light = {n: tan[n] for n in ("x0", "xref", "gd", "fz_min")}
    base = _jvp(plan, case, light)
    assert np.abs(base).max() > 0.0
    for n in ("Q", "R", "mu", "Ad", "Bd"):
        assert np.array_equal(base, _jvp(plan, case, dict(light, **{n: zeros[n]}))), n
    assert np.array_equal(base, _jvp(plan, case, dict(zeros, **light)))
    assert np.all(_jvp(plan, case, zeros) == 0.0)


@pytest.mark.parametrize("N", [1, 5, 16])
def test_arbitrary_face_sets_given(N):
    from cmpc import Plan, SolverParams, _lib
    plan = Plan(SolverParams(N=N, max_batch=8))     # (max_batch does not limit B)
    c, faces, nan_rows = random_case(N)
    B = len(faces)
    th = dict(_theta(c, plan.params), mu=np.abs(c["mu"]), R=np.abs(c["R"]))
    tan = jvp_util.random_tangents(np.random.default_rng(31 + N), th)
    good = [i for i in range(B) if i not in nan_rows]
    dev = _jvp(plan, c, tan, use_w=False, faces=faces)
    assert np.all(np.isnan(dev[nan_rows])) and np.all(np.isfinite(dev[good]))
    dense = set(range(0, B, 4)) | {0, 1, 2}
    _check(dev, c, faces, tan, plan.params, good, dense & set(good), f"N={N} B={B}")
    # smaller batches of the same instances: bitwise the same rows (independent of B and place)
    for idx in ([2, 5, 6], [0], [5], [3]):
        idx = np.array(idx)
        sub = _jvp(plan, c, tan, idx=idx, use_w=False, faces=faces)
        assert np.array_equal(sub, dev[idx], equal_nan=True), idx
    # a struct that ends right after dw, through raw ctypes
    t = {k: _dev(plan, c[k]) for k in IN + ("mu", "fz_min", "Q", "R")}
    t["faces"] = _dev(plan, faces)
    t.update({"d_" + n: _dev(plan, v) for n, v in tan.items()})
    out = torch.zeros((B, 24 * N), dtype=torch.float64, device=plan.device)
    io = _lib.CJvpIO()
    for k, v in t.items():
        setattr(io, k, v.data_ptr())
    io.dw = out.data_ptr()
    io.size = _lib.CJvpIO.dw.offset + ctypes.sizeof(ctypes.c_void_p)
    with torch.cuda.device(plan.device):
        rc = plan.lib.cmpc_jvp_run(plan._h, ctypes.c_int64(B), ctypes.byref(io), ctypes.c_void_p(
            torch.cuda.current_stream(plan.device).cuda_stream))
    torch.cuda.synchronize(plan.device)
    assert rc == 0, _lib.last_error(plan.lib)
    assert np.array_equal(out.cpu().numpy(), dev, equal_nan=True)
    plan.close()


def _cfg2(plan):
    case, faces = _fixture(plan, "qp_cfg2.npz", "")
    idx = np.arange(0, 64, 4)
    sub = {k: v[idx] for k, v in case.items() if isinstance(v, np.ndarray)}
    return sub, faces[idx]


def test_x0_tangent_is_a_column_of_the_gain(plan):
    """d_x0 = e_j: the first 12 force entries of dw are column j of Plan.gain's K, on 16
    instances of qp_cfg2, within 2e-8 x max(1, max|K|) (each side's own bar)."""
    case, faces = _cfg2(plan)
    N = plan.params.N
    t = [_dev(plan, case[k]) for k in IN]
    K = plan.gain(*t, faces=_dev(plan, faces))["K"].cpu().numpy()
    worst = 0.0
    for j in range(12):
        d = np.zeros((len(faces), 12), np.float32)
        d[:, j] = 1.0
        du0 = _jvp(plan, case, dict(x0=d), use_w=False, faces=faces)[:, 12 * N:12 * N + 12]
        worst = max(worst, float(np.max(np.abs(du0 - K[:, :, j]).max(axis=1) /
                                        (2e-8 * np.maximum(1.0, np.abs(K).max(axis=(1, 2)))))))
    print("worst |du_0 - K[:, j]| / (2e-8 max(1, max|K|)):", worst)
    assert worst <= 1.0


def test_finite_steps_in_xref_gd_x0(plan):
    """With the faces fixed u_star is affine in (xref, gd, x0): u_star(theta + d) - u_star(theta)
    is the force part of dw for d_theta = d, for displacements that are not small.  theta and d
    lie on a grid of 2^-10 so that theta + d is exact in fp32.  Tolerance: the sum of the bars --
    each u_star within 1e-8 x max|u| of its exact value, du within 1e-8 x S_u."""
    case, faces = _cfg2(plan)
    N = plan.params.N
    B = len(faces)
    grid = lambda v: kkt_util.f32(np.round(np.asarray(v, np.float64) * 1024.0) / 1024.0)  # noqa: E731
    case = dict(case, **{n: grid(case[n]) for n in ("xref", "gd", "x0")})

    def u_star(c):
        out = plan.gain(*[_dev(plan, c[k]) for k in IN], faces=_dev(plan, faces),
                        want=("K", "u_star"))["u_star"]
        return out.cpu().numpy()
    u0 = u_star(case)
    rng = np.random.default_rng(9)
    worst = 0.0
    for size in (0.05, 0.5, 3.0):
        for n in ("xref", "gd", "x0"):
            d = grid(size * rng.uniform(-1.0, 1.0, case[n].shape))
            moved = dict(case, **{n: case[n] + d})
            assert np.array_equal(moved[n].astype(np.float64),
                                  case[n].astype(np.float64) + d.astype(np.float64))
            assert np.abs(d).max() > 0.5 * size
            u1 = u_star(moved)
            du = _jvp(plan, case, {n: d}, use_w=False, faces=faces)[:, 12 * N:]
            S_u = np.array([_refs(case, faces, {n: d}, plan.params, i)[2] for i in range(B)])
            umax = np.maximum(np.abs(u1).max(axis=1), np.abs(u0).max(axis=1))
            tol = vjp_util.TOL_REL * (2.0 * umax + S_u)
            ratio = np.abs((u1 - u0) - du).max(axis=1) / tol
            print("size", size, n, "max |du|", np.abs(du).max(), "worst / tol", ratio.max())
            worst = max(worst, ratio.max())
    assert worst <= 1.0


def test_adjoint_identity_against_plan_vjp(plan):
    """gw . dw (Plan.jvp) = sum_theta g_theta . d_theta (Plan.vjp) on 16 instances of qp_cfg2,
    faces given, gw and the nine tangents random: within the sum of both sides' bars,
    1e-8 x (sum |gw| S_w + sum_theta S_theta |d_theta|_1)."""
    case, faces = _cfg2(plan)
    B, N = len(faces), plan.params.N
    rng = np.random.default_rng(12)
    tan = jvp_util.random_tangents(rng, _theta(case, plan.params))
    gw = vjp_util.random_gw(rng, (B, 24 * N))
    dw = _jvp(plan, case, tan, use_w=False, faces=faces)
    g = plan.vjp(*[_dev(plan, case[k]) for k in IN], _dev(plan, gw), faces=_dev(plan, faces),
                 want=ALL)
    g = {n: v.cpu().numpy() for n, v in g.items()}
    worst = 0.0
    for i in range(B):
        iv = kkt_util.instance_values(case, i, plan.params)
        args, kw = gain_util.instance_args(case, i, iv)
        S = vjp_util.ref_riccati(*args, faces[i], gw=gw[i], **kw)[1]
        _, S_x, S_u, _ = _refs(case, faces, tan, plan.params, i)
        a = np.abs(gw[i].astype(np.float64))
        lhs = float(gw[i].astype(np.float64) @ dw[i])
        rhs = sum(float(np.sum(g[n][i] * tan[n][i].astype(np.float64))) for n in ALL)
        tol = vjp_util.TOL_REL * (S_x * a[:12 * N].sum() + S_u * a[12 * N:].sum() +
                                  sum(S[n] * float(np.abs(tan[n][i]).sum()) for n in ALL))
        assert abs(lhs) > 0.0
        worst = max(worst, abs(lhs - rhs) / tol)
    print("worst |gw . dw - sum g . d| / tol:", worst)
    assert worst <= 1.0


def test_repeatable_and_position_independent(plan):
    case, faces, tan = _fixture_tan(plan, "qp_terrain.npz", "_A")
    a, b = _jvp(plan, case, tan), _jvp(plan, case, tan)
    assert np.array_equal(a, b)
    rev = {k: (v[::-1].copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    r = _jvp(plan, rev, {n: v[::-1].copy() for n, v in tan.items()})
    assert np.array_equal(r[::-1], a)
    perm = np.random.default_rng(1).permutation(len(faces))
    assert np.array_equal(_jvp(plan, case, tan, idx=perm), a[perm])
    # and a tile of the batch past one grid-stride pass of the kernel (8192 blocks)
    reps = 8192 // len(faces) + 2
    tile = lambda v: np.tile(v, (reps,) + (1,) * (v.ndim - 1))  # noqa: E731
    big = _jvp(plan, {k: tile(v) for k, v in case.items() if isinstance(v, np.ndarray)},
               {n: tile(v) for n, v in tan.items()})
    assert np.array_equal(big, tile(a))


def test_forward_mode_autograd(plan):
    """cmpc.autograd.solve under torch.autograd.forward_ad on 64 instances of config 2, x0 and
    the per-robot mu, Q carrying tangents: the tangent of w is Plan.jvp's result on w's faces
    cast to fp32, zero in the row of status -10; cmpc.autograd.jvp is the functional form."""
    import torch.autograd.forward_ad as fwAD
    from cmpc import autograd, synth, to_device_batch
    B = 64
    d = to_device_batch(synth.make_config(2, B=B), plan.device)
    args = [d[k] for k in IN]
    p = plan.params
    f32 = dict(dtype=torch.float32, device=plan.device)
    per = dict(mu=torch.full((B,), p.mu, **f32), fz_min=torch.full((B,), p.fz_min, **f32),
               Q=torch.tensor(p.Q, **f32).repeat(B, 1), R=torch.tensor(p.R, **f32).repeat(B, 1))
    per["mu"][3] = -1.0                                    # an invalid entry: status -10
    gen = torch.Generator().manual_seed(5)
    tan = dict(x0=torch.randn(B, 12, generator=gen).to(plan.device),
               mu=(0.1 * torch.randn(B, generator=gen)).to(plan.device),
               Q=torch.randn(B, 12, generator=gen).to(plan.device))
    asked = []
    jvp = plan.jvp
    plan.jvp = lambda *a, **k: asked.append(tuple(a[6])) or jvp(*a, **k)
    try:
        with fwAD.dual_level():
            call = args[:3] + [fwAD.make_dual(args[3], tan["x0"])] + args[4:]
            duals = dict(per, mu=fwAD.make_dual(per["mu"], tan["mu"]),
                         Q=fwAD.make_dual(per["Q"], tan["Q"]))
            w, st, it = autograd.solve(plan, *call, **duals)
            wp, wt = fwAD.unpack_dual(w)
            assert fwAD.unpack_dual(st).tangent is None and fwAD.unpack_dual(it).tangent is None
    finally:
        del plan.jvp
    assert asked == [("x0", "mu", "Q")]                    # exactly what carries a tangent
    assert int(st[3]) == -10 and bool(torch.all(st[torch.arange(B) != 3] > 0))
    ref = plan.jvp(*args, tan, w=wp, **per)
    torch.cuda.synchronize(plan.device)
    assert bool(torch.isnan(ref[3]).all())                 # the entry's own answer there: NaN
    want = ref.to(torch.float32)
    want[3] = 0.0                                          # the layer's: no tangent
    assert wt.dtype == wp.dtype and wt.shape == wp.shape and torch.equal(wt, want)
    assert bool(torch.all(torch.isfinite(wt))) and float(wt.abs().max()) > 0.0
    # the functional form: the same on its own solve's faces
    w2, st2, _, t2 = autograd.jvp(plan, *args, dict(x0=tan["x0"]), **per)
    only = plan.jvp(*args, dict(x0=tan["x0"]), w=w2, **per).to(torch.float32)
    only[3] = 0.0
    assert int(st2[3]) == -10 and torch.equal(t2, only) and float(t2.abs().max()) > 0.0
    # without a tangent nothing is launched
    plan.jvp = lambda *a, **k: asked.append("called") or jvp(*a, **k)
    try:
        with fwAD.dual_level():
            w3 = autograd.solve(plan, *args, **per)[0]
            assert fwAD.unpack_dual(w3).tangent is None
    finally:
        del plan.jvp
    assert asked == [("x0", "mu", "Q")]


def test_graph_capture(plan):
    """One Plan.jvp call captured in a torch.cuda.graph, replayed on another tangent written in
    place: bitwise the eager call."""
    case, faces, tan = _fixture_tan(plan, "qp_cfg2.npz", "")
    B, N = len(faces), plan.params.N
    t = [_dev(plan, case[k]) for k in IN]
    w = _dev(plan, case["w"])
    d1 = {n: _dev(plan, v) for n, v in tan.items()}
    other = jvp_util.random_tangents(np.random.default_rng(4), _theta(case, plan.params))
    d2 = {n: _dev(plan, v) for n, v in other.items()}
    buf = {n: v.clone() for n, v in d1.items()}
    out = torch.empty((B, 24 * N), dtype=torch.float64, device=plan.device)
    side = torch.cuda.Stream(plan.device)
    side.wait_stream(torch.cuda.current_stream(plan.device))
    with torch.cuda.stream(side):
        plan.jvp(*t, buf, w=w, out=out)                     # (warm-up on the capture stream)
    torch.cuda.current_stream(plan.device).wait_stream(side)
    torch.cuda.synchronize(plan.device)
    first = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.jvp(*t, buf, w=w, out=out)
    for n in buf:
        buf[n].copy_(d2[n])
    out.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize(plan.device)
    eager = plan.jvp(*t, d2, w=w)
    torch.cuda.synchronize(plan.device)
    assert torch.equal(out, eager) and not torch.equal(first, eager)
