"""CPU: the test infrastructure of tests/test_gpu_traj_grad.py and the host side of
cmpc_traj_vjp_run / cmpc_traj_jvp_run (include/cmpc.h).

traj_grad_util's smooth function is tied to oracle.traj_ref.generate_traj, its two derivative
references to torch.autograd on a float64 restatement, to each other (the adjoint identity) and
to central differences of the oracle, and the composition  cmd, x0 -> trajectory -> dynamics ->
optimum on the held faces -> loss  to central differences in float64.  The io structs are checked
against their ctypes mirrors.

Measured worst ratios to the bars (N = 1, 5, 16 at 67 robots): forward against the oracle 8.2e-3
of 1e-13 S; the references against torch.autograd 2.2e-3 (vjp) and 2.0e-3 (jvp) of 1e-13 S; the
adjoint identity 1.1e-3 of 1e-13 sum|.||.|; ref_jvp against central differences of the oracle
1.7e-3 of 1e-7 S; the composition 0.33 of 1e-6 sum|g||d| (one attitude direction; 0.045 and less
for the other five)."""
import ctypes
import functools
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from parity_util import load_fixture
import dyn_grad_util as dg
import gain_util
import kkt_util
import traj_grad_util as tg
import vjp_util

HORIZONS = [1, 5, 16]
B_CPU = 67


@functools.lru_cache(maxsize=None)
def _case(N):
    return tg.random_case(np.random.default_rng(70 + N), B_CPU, N)


def _oracle(c, **moved):
    """oracle.traj_ref.generate_traj on the case's inputs (widened exactly), ``moved`` replacing
    some -> (pos_des', xref, r_feet)."""
    from oracle import traj_ref
    a = {k: np.asarray(c[k], np.float64) for k in ("x0", "pos_des", "cmd", "t_now", "gait",
                                                   "foot_lever", "hip")}
    a.update(moved)
    pd, xref, _, r = traj_ref.generate_traj(a["x0"], a["pos_des"], a["cmd"], a["t_now"], a["gait"],
                                            a["foot_lever"], a["hip"], c["dt"], c["N"])
    return dict(pos_des=pd, xref=xref, r_feet=r)


@pytest.mark.parametrize("N", HORIZONS)
def test_inputs_meet_the_conditions(N):
    """What the other tests rely on: every clamp branch on each axis, no robot within 1e-4 of a
    branch, and the lever classes that the horizon can have."""
    from cmpc import Plan, autograd
    assert callable(Plan.traj_vjp) and callable(Plan.traj_jvp) and callable(autograd.generate_traj)
    c = _case(N)
    gap = c["pos_des"][:, :2] - np.float64(c["x0"][:, :2])
    for a in range(2):
        assert (gap[:, a] > 0.1).any() and (gap[:, a] < -0.1).any() and (np.abs(gap[:, a]) < 0.1).any()
    assert np.abs(np.abs(gap) - 0.1).min() > 1e-4
    cls, _ = tg.classes(c["t_now"], c["gait"], c["dt"], N)
    want = {tg.SWING, tg.CURRENT} if N == 1 else {tg.SWING, tg.CURRENT, tg.PREDICTED}
    assert set(np.unique(cls)) == want


@pytest.mark.parametrize("N", HORIZONS)
def test_forward_is_the_oracles(N):
    """traj_grad_util.forward against oracle.traj_ref.generate_traj within 1e-13 x S, and the lever
    classes read off the oracle's levers: 0 in swing, the current lever (bitwise) in class C,
    anything else in class P."""
    c = _case(N)
    vals, S, cls = tg.forward(*[c[k] for k in ("x0", "pos_des", "cmd", "t_now", "gait", "foot_lever",
                                               "hip")], c["dt"], N)
    ref = _oracle(c)
    worst = tg.worst_ratio(vals, ref, S, tol=1e-13)
    print("N", N, "worst |util - oracle| / (1e-13 S):", worst)
    assert max(worst.values()) <= 1.0
    r = ref["r_feet"]
    fl = np.broadcast_to(np.float64(c["foot_lever"])[:, None], r.shape)
    swing = np.all(r == 0.0, axis=-1)
    current = np.all(r == fl, axis=-1) & ~swing
    read = np.where(swing, tg.SWING, np.where(current, tg.CURRENT, tg.PREDICTED))
    assert np.array_equal(read, cls)


def _torch_forward(torch, c):
    """The smooth function restated in float64 torch ops, classes and clamp branches held fixed:
    (x0, pos_des, cmd, foot_lever) -> (xref, r_feet, pos_des')."""
    N, dt = c["N"], c["dt"]
    q = tg._leaves(*[c[k] for k in tg.INPUTS], dt, N)
    T = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64)  # noqa: E731
    sigma, sign = T(q.sigma), T(np.sign(q.pd[:, :2] - q.p))
    P, C, tj, tk, tau = T(q.P), T(q.C), T(q.tj), T(q.tk), T(q.tau)
    hip = T(tg.f32(c["hip"]))

    def f(x0, pos_des, cmd, fl):
        B = x0.shape[0]
        vxb, vyb, zdes, wz = cmd.unbind(1)
        phi, th, psi = x0[:, 3], x0[:, 4], x0[:, 5]
        c_, s_ = torch.cos(psi), torch.sin(psi)
        pd = sigma * (x0[:, 0:2] + 0.1 * sign) + (1.0 - sigma) * pos_des[:, 0:2]
        vwx, vwy = c_ * vxb - s_ * vyb, s_ * vxb + c_ * vyb
        z = torch.zeros(B, N, dtype=torch.float64)
        col = lambda v: v[:, None] + z                                       # noqa: E731
        xref = torch.stack([pd[:, 0:1] + vwx[:, None] * tk, pd[:, 1:2] + vwy[:, None] * tk,
                            col(zdes), z, z, psi[:, None] + wz[:, None] * tk, col(vwx), col(vwy),
                            z, z, z, col(wz)], -1)
        cr, sr, cp, sp = torch.cos(phi), torch.sin(phi), torch.cos(th), torch.sin(th)
        vbx = (c_ * cp) * vwx + (s_ * cp) * vwy
        vby = (c_ * sp * sr - s_ * cr) * vwx + (s_ * sp * sr + c_ * cr) * vwy
        b = lambda v: v[:, None, None]                                       # noqa: E731
        psij = b(psi) + b(wz) * tj
        hwx = torch.cos(psij) * hip[:, 0] - torch.sin(psij) * hip[:, 1]
        hwy = torch.sin(psij) * hip[:, 0] + torch.cos(psij) * hip[:, 1]
        r = torch.stack([hwx + b(vbx * tau) - b(wz * tau) * hwy, hwy + b(vby * tau) + b(wz * tau) * hwx,
                         (0.02 - b(zdes)) + 0.0 * hwx], -1)
        r = r * P[..., None] + fl[:, None] * C[..., None]
        return xref, r, torch.cat([pd, zdes[:, None]], 1)
    return f


@pytest.mark.parametrize("N", HORIZONS)
def test_references_equal_torch_autograd(N):
    """ref_vjp and ref_jvp against torch.autograd.grad and torch.autograd.functional.jvp of the
    float64 restatement: within 1e-13 x S (the bar of test_dyn_grad.py for the same comparison)."""
    import torch
    c = _case(N)
    f = _torch_forward(torch, c)
    lead = [torch.tensor(tg.f32(c["x0"]), requires_grad=True),
            torch.tensor(c["pos_des"], requires_grad=True),
            torch.tensor(tg.f32(c["cmd"]), requires_grad=True),
            torch.tensor(tg.f32(c["foot_lever"]), requires_grad=True)]
    xref, r, pd = f(*lead)
    vals, S, _ = tg.forward(*[c[k] for k in ("x0", "pos_des", "cmd", "t_now", "gait", "foot_lever",
                                             "hip")], c["dt"], N)
    got = dict(xref=xref.detach().numpy(), r_feet=r.detach().numpy(), pos_des=pd.detach().numpy())
    assert max(tg.worst_ratio(got, vals, S, tol=1e-13).values()) <= 1.0   # the restatement is the function
    G = torch.tensor(c["g_xref"]).clone()
    G[:, :, 5] += torch.tensor(c["g_yaw"] / N)[:, None]
    loss = (xref * G).sum() + (r * torch.tensor(c["g_r_feet"])).sum() + (pd * torch.tensor(c["g_pos_des"])).sum()
    gx, gp, gc, gf = (g.numpy() for g in torch.autograd.grad(loss, lead))
    v, Sv = tg.ref_vjp(*tg.inputs(c), **tg.gradients(c))
    worst = tg.worst_ratio(dict(x0=gx, pos_des=gp, cmd=gc, foot_lever=gf), v, Sv, tol=1e-13)
    tan = (torch.tensor(tg.f32(c["d_x0"])), torch.tensor(c["d_pos_des"]),
           torch.tensor(tg.f32(c["d_cmd"])), torch.tensor(tg.f32(c["d_foot_lever"])))
    _, (dx, dr, dp) = torch.autograd.functional.jvp(f, tuple(t.detach() for t in lead), tan)
    j, Sj = tg.ref_jvp(*tg.inputs(c), **tg.tangents(c))
    jworst = tg.worst_ratio(dict(xref=dx.numpy(), r_feet=dr.numpy(), pos_des=dp.numpy()), j, Sj, tol=1e-13)
    print("N", N, "worst |ref - torch| / (1e-13 S): vjp", worst, "jvp", jworst)
    # (a robot with every lever in swing has S = 0 and an exactly zero row in the lever outputs)
    assert all(np.all(s > 0.0) for s in (Sv["x0"], Sv["cmd"], Sj["xref"], Sj["pos_des"]))
    assert max(worst.values()) <= 1.0 and max(jworst.values()) <= 1.0
    assert np.all(v["x0"][:, [2, 6, 7, 8, 9, 10, 11]] == 0.0) and np.all(v["pos_des"][:, 2] == 0.0)


def _pairs(c, g, d):
    """(gradient, tangent) pairs of the adjoint identity: outputs' side, then inputs' side."""
    N = c["N"]
    G = c["g_xref"].copy()
    G[:, :, 5] += (c["g_yaw"] / N)[:, None]
    left = [(G, d["xref"]), (c["g_r_feet"], d["r_feet"]), (c["g_pos_des"], d["pos_des"])]
    right = [(g["x0"], tg.f32(c["d_x0"])), (g["pos_des"], c["d_pos_des"]),
             (g["cmd"], tg.f32(c["d_cmd"])), (g["foot_lever"], tg.f32(c["d_foot_lever"]))]
    return left, right


@pytest.mark.parametrize("N", HORIZONS)
def test_adjoint_identity_of_the_references(N):
    """<G, d_xref> + <H, d_r_feet> + <gp, d_pos_des'> = <g_x0, d_x0> + <g_pos_des, d_pos_des> +
    <g_cmd, d_cmd> + <g_foot_lever, d_foot_lever> per robot, within 1e-13 x the sum of
    |factor| |factor| over both sides."""
    c = _case(N)
    g, _ = tg.ref_vjp(*tg.inputs(c), **tg.gradients(c))
    d, _ = tg.ref_jvp(*tg.inputs(c), **tg.tangents(c))
    left, right = _pairs(c, g, d)
    B = B_CPU
    dot = lambda ps: sum((x * y).reshape(B, -1).sum(1) for x, y in ps)       # noqa: E731
    mag = sum((np.abs(x) * np.abs(y)).reshape(B, -1).sum(1) for x, y in left + right)
    ratio = np.abs(dot(left) - dot(right)) / (1e-13 * mag)
    print("N", N, "worst adjoint mismatch / (1e-13 sum|.||.|):", float(ratio.max()))
    assert np.all(mag > 0.0) and ratio.max() <= 1.0


@pytest.mark.parametrize("N", HORIZONS)
def test_jvp_equals_central_differences_of_the_oracle(N):
    """ref_jvp against (f(u + h d) - f(u - h d)) / 2h of oracle.traj_ref.generate_traj, the
    direction d random in x0, pos_des, cmd and foot_lever at once, h = 1e-5: within 1e-7 x S.
    The quotient's own error is about h^2/6 |f'''| <~ 1e-9 x S (|wz| <= 4, t <= 0.5) and rounding
    adds about 40 x 1.1e-16 x S / h = 4e-10 x S; a wrong or missing term is O(1) x S.  Measured
    worst ratio 1.7e-3 (d_xref at N = 5)."""
    c = _case(N)
    h = 1e-5
    d = {k: np.asarray(c["d_" + k], np.float64) for k in tg.JVP_TANGENTS}
    side = lambda s: _oracle(c, **{k: np.asarray(c[k], np.float64) + s * h * d[k] for k in d})  # noqa: E731
    up, dn = side(1.0), side(-1.0)
    fd = {k: (up[k] - dn[k]) / (2.0 * h) for k in up}
    vals, S = tg.ref_jvp(*tg.inputs(c), **tg.tangents(c))
    worst = tg.worst_ratio(fd, vals, S, tol=1e-7)
    print("N", N, "worst |fd - ref_jvp| / (1e-7 S):", worst)
    assert max(worst.values()) <= 1.0


def _w_star_refined(Ad, Bd, gd, x0, xref, contact, faces, Q, R, mu, fz_min):
    """vjp_util.w_star -- its KKT system, its least-squares solve -- followed by two steps of
    iterative refinement with the residual in extended precision.  The plain solve leaves about
    2.5e-10 of rounding in L (|L| ~ 1e3, the KKT matrix's condition ~ 1e6); over a step of 5e-6
    that is 2.5e-5 in the quotient, above the bar of the attitude direction, whose
    sum |g_i| |d_i| is about 10."""
    import scipy.linalg
    Ad, Bd, gd, x0, xref, Q, R = vjp_util._f64(Ad, Bd, gd, x0, xref, Q, R)
    kkt, rhs, n, _ = vjp_util._kkt(Ad, Bd, gd, x0, xref, contact, faces, Q, R, float(mu), float(fz_min))
    solve = lambda r: scipy.linalg.lstsq(kkt, r, lapack_driver="gelsy")[0]   # noqa: E731
    z = solve(rhs)
    wide = kkt.astype(np.longdouble)
    for _ in range(2):
        z = z + solve(np.asarray(rhs - wide @ z, np.float64))
    return z[:n]


def test_composition_equals_central_differences():
    """L = c . w*(Ad, Bd, xref) with (xref, r_feet) = generate_traj(x0, cmd, ..) and (Ad, Bd) the
    dynamics of those, on three instances of the config-2 fixture (its x0, contact, weights and
    the faces read off its fp32 w; tick inputs of make_tick_inputs).  g_cmd and g_x0[3:6] of the
    chained references  vjp_util.ref_dense -> dyn_grad_util.ref_vjp -> traj_grad_util.ref_vjp
    against central differences of  oracle.traj_ref -> dyn_grad_util forward -> w*  along a random
    direction in cmd and one in x0[3:6]: within 1e-6 x sum |g_i| |d_i|, the step from 1e-5 halved
    until halving moves the quotient by less than the bar (test_dyn_grad.py's rule).  Measured
    worst ratio 0.33 (the attitude direction of instance 0, step 5e-6; the other five 0.045 and
    less)."""
    from cmpc import SolverParams, synth
    from oracle import traj_ref
    params = SolverParams()
    N = params.N
    case = kkt_util.fixture_case(load_fixture("qp_cfg2.npz"), "", params)
    nB = len(case["w"])
    b = synth.make_config(2, B=nB)
    t = synth.make_tick_inputs(nB, seed=61, mixed=True, N=N)
    dt = float(np.float32(t["dt"]))                     # (the dynamics entry's dt is a float)
    m, I = dg.f32(b["m"]), dg.f32(b["I_world"])
    rng = np.random.default_rng(62)
    worst = 0.0
    for i in (0, 21, 42):
        one = lambda a: np.asarray(a, np.float64)[i:i + 1]                  # noqa: E731
        tick = {k: one(t[k]) for k in ("x0", "pos_des", "cmd", "t_now", "gait", "foot_lever")}
        iv = kkt_util.instance_values(case, i, params)
        contact = case["contact"][i]
        faces = gain_util.classify(contact, case["w"][i], iv["mu"], iv["fz_min"])
        gd, x0qp = (case[k][i].astype(np.float64) for k in ("gd", "x0"))
        tail = (contact, faces, iv["Q"], iv["R"], iv["mu"], iv["fz_min"])
        cvec = rng.standard_normal(24 * N)

        def stages(x0, cmd):
            _, xref, _, r = traj_ref.generate_traj(x0, tick["pos_des"], cmd, tick["t_now"],
                                                   tick["gait"], tick["foot_lever"], t["hip"], dt, N)
            return xref, r

        def loss(x0, cmd):
            xref, r = stages(x0, cmd)
            A1, B1 = dg._forward64(one(m), one(I), r, xref, dt)
            return float(cvec @ _w_star_refined(A1[0], B1[0], gd, x0qp, xref[0], *tail))

        # the chained references, at the fp32 roundings of xref and r_feet that dyn_grad_util takes
        xref, r = stages(tick["x0"], tick["cmd"])
        xr32, r32 = dg.f32(xref), dg.f32(r)
        Ad, Bd = dg._forward64(one(m), one(I), r32, xr32, dt)
        vals, _ = vjp_util.ref_dense(Ad[0], Bd[0], gd, x0qp, xr32[0], *tail, cvec)
        gdyn, _ = dg.ref_vjp(one(m), one(I), r32, xr32, dt, vals["Ad"][None], vals["Bd"][None])
        g, _ = tg.ref_vjp(tick["x0"], tick["pos_des"], tick["cmd"], tick["t_now"], tick["gait"],
                          t["hip"], dt, N, g_xref=vals["xref"][None], g_r_feet=gdyn["r_feet"],
                          g_yaw=gdyn["yaw"])
        d_cmd = rng.standard_normal(4)
        d_rpy = rng.standard_normal(3)
        e = np.zeros(12)
        e[3:6] = d_rpy
        for name, gvec, dvec, move in (
                ("cmd", g["cmd"][0], d_cmd, lambda s: (tick["x0"], tick["cmd"] + s * d_cmd)),
                ("x0[3:6]", g["x0"][0, 3:6], d_rpy, lambda s: (tick["x0"] + s * e, tick["cmd"]))):
            bar = 1e-6 * float(np.sum(np.abs(gvec) * np.abs(dvec)))
            fd = lambda h: (loss(*move(h)) - loss(*move(-h))) / (2.0 * h)    # noqa: E731
            h = 1e-5
            cur = fd(h)
            for _halvings in range(6):
                nxt = fd(0.5 * h)
                moved, cur, h = abs(nxt - cur), nxt, 0.5 * h
                if moved < bar:
                    break
            assert moved < bar, (i, name, h, moved, bar)
            ratio = abs(cur - float(gvec @ dvec)) / bar
            worst = max(worst, ratio)
            print("instance", i, name, "step", h, "fd", cur, "g . d", float(gvec @ dvec), "ratio", ratio)
    print("worst |fd - g . d| / (1e-6 sum|g||d|):", worst)
    assert worst <= 1.0


def test_struct_layouts_match_header(tmp_path):
    """sizeof / offsetof of cmpc_traj_vjp_io and cmpc_traj_jvp_io as a C compiler lays out
    include/cmpc.h; the ABI version did not move."""
    from cmpc import _lib
    from cmpc.build import hipcc
    structs = (("cmpc_traj_vjp_io", _lib.CTrajVjpIO), ("cmpc_traj_jvp_io", _lib.CTrajJvpIO))
    body = '  printf("%d\\n", CMPC_ABI_VERSION);\n'
    for cname, mirror in structs:
        body += f'  printf("%zu\\n", sizeof({cname}));\n'
        body += "".join(f'  printf("%zu\\n", offsetof({cname}, {n}));\n' for n, _ in mirror._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cmpc.h"\nint main(void) {\n' +
                   body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    cc = shutil.which("cc") or shutil.which("gcc")
    cmd = [cc, str(src)] if cc else [hipcc(), "-x", "c", str(src)]
    subprocess.run(cmd + [f"-I{REPO / 'include'}", "-o", str(exe)], check=True, timeout=120)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True,
                                           timeout=60).stdout.split()]
    want = [_lib.ABI_VERSION]
    for _, mirror in structs:
        want += [ctypes.sizeof(mirror)] + [getattr(mirror, n).offset for n, _ in mirror._fields_]
    assert vals == want and vals[0] == 6
    head = ["size", "x0", "pos_des", "cmd", "t_now", "gait", "hip", "dt"]
    assert [n for n, _ in _lib.CTrajVjpIO._fields_] == head + [
        "g_xref", "g_r_feet", "g_yaw", "g_pos_des_out", "g_x0", "g_pos_des", "g_cmd", "g_foot_lever"]
    assert [n for n, _ in _lib.CTrajJvpIO._fields_] == head + [
        "d_x0", "d_pos_des", "d_cmd", "d_foot_lever", "d_xref", "d_r_feet", "d_pos_des_out"]
    assert _lib.TRAJ_VJP_OUTPUTS == tg.VJP_OUTPUTS
    assert _lib.TRAJ_JVP_TANGENTS == tg.JVP_TANGENTS and _lib.TRAJ_JVP_OUTPUTS == tg.JVP_OUTPUTS


def test_argument_checks_that_need_no_plan():
    """A null io and a size that does not reach the first output are refused before the plan is
    touched; the entries are declared and exported."""
    from cmpc import _lib
    from cmpc.build import build_library, LIB
    from test_cabi import declared_symbols
    if not LIB.exists():
        build_library()
    lib = _lib.load()
    for entry, mirror, first in (("cmpc_traj_vjp_run", _lib.CTrajVjpIO, "g_x0"),
                                 ("cmpc_traj_jvp_run", _lib.CTrajJvpIO, "d_xref")):
        assert entry in declared_symbols() and entry in _lib.EXPORTS and hasattr(lib, entry)
        fn = getattr(lib, entry)
        assert fn(None, 1, None, None) == -22 and "null io" in _lib.last_error(lib)
        io = mirror()
        io.size = getattr(mirror, first).offset          # ends just before the first output
        assert fn(None, 1, ctypes.byref(io), None) == -22
        assert "size" in _lib.last_error(lib) and entry in _lib.last_error(lib)
        io.size = ctypes.sizeof(mirror)
        assert fn(None, 1, ctypes.byref(io), None) == -22 and "null plan" in _lib.last_error(lib)
