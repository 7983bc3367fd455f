"""CPU: the test infrastructure of tests/test_gpu_dyn_grad.py and the host side of
cmpc_dynamics_vjp_run / cmpc_dynamics_jvp_run (include/cmpc.h).

dyn_grad_util's closed form is tied to the project's (cmpc.synth), its two derivative references
to torch.autograd on a float64 restatement and to each other (the adjoint identity), and the
composition  r_feet -> dynamics -> optimum on the held faces -> loss  to central differences in
float64.  The io structs are checked against their ctypes mirrors."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from parity_util import load_fixture
import dyn_grad_util as dg
import gain_util
import kkt_util
import vjp_util


@pytest.fixture(scope="module")
def base():
    from cmpc import synth
    return synth.make_config(3, B=64)


def test_forward_is_the_projects_closed_form(base):
    """dyn_grad_util.forward on the fp32-rounded inputs against cmpc.synth's Ad and Bd, at the bar
    of test_gpu_dynamics: one fp32 rounding of the entry plus 4e-7 of the array's largest."""
    from cmpc import Plan, autograd
    from test_gpu_dynamics import _close
    assert callable(Plan.dynamics_vjp) and callable(Plan.dynamics_jvp)
    assert callable(autograd.build_dynamics)
    Ad, Bd = dg.forward(base["m"], base["I_world"], base["r_legs"], base["xref"], base["dt"])
    assert _close(Ad, base["Ad"]) and _close(Bd, base["Bd"])
    assert np.abs(Bd).max() > 0.0


def _skew_t(torch, r):
    z = torch.zeros_like(r[..., 0])
    return torch.stack([torch.stack([z, -r[..., 2], r[..., 1]], -1),
                        torch.stack([r[..., 2], z, -r[..., 0]], -1),
                        torch.stack([-r[..., 1], r[..., 0], z], -1)], -2)


def _torch_forward(torch, dt):
    """The closed form restated in float64 torch ops: (mass, inertia, r_feet, xref) -> (Ad, Bd)."""
    def f(mass, inertia, r_feet, xref):
        B, N = r_feet.shape[:2]
        h2 = 0.5 * dt * dt
        J = torch.linalg.inv(inertia)
        yaw = xref[:, :, 5].sum(1) / N
        c, s, z, o = torch.cos(yaw), torch.sin(yaw), torch.zeros_like(yaw), torch.ones_like(yaw)
        Rt = torch.stack([torch.stack([c, s, z], -1), torch.stack([-s, c, z], -1),
                          torch.stack([z, z, o], -1)], -2)
        W = torch.einsum("bij,bkljm->bklim", J, _skew_t(torch, r_feet))
        V = torch.einsum("bij,bkljm->bklim", Rt, W)
        eye = torch.eye(3, dtype=mass.dtype).expand(B, N, 4, 3, 3) / mass[:, None, None, None, None]
        # (B, N, leg, q, i, j) -> rows 3q + i, columns 3 leg + j
        Bd = torch.stack([h2 * eye, h2 * V, dt * eye, dt * W], 3)
        Bd = Bd.permute(0, 1, 3, 4, 2, 5).reshape(B, N, 12, 12)
        const = np.eye(12)
        const[0:3, 6:9] += dt * np.eye(3)
        Ad = torch.tensor(const) + torch.nn.functional.pad(dt * Rt, (9, 0, 3, 6))  # rows 3-5, cols 9-11
        return Ad, Bd
    return f


@pytest.mark.parametrize("N", [1, 5, 16])
def test_references_equal_torch_autograd(base, N):
    """ref_vjp and ref_jvp against torch.autograd.grad and torch.autograd.functional.jvp of the
    float64 restatement, 8 robots, random g_Ad, g_Bd and tangents: within 1e-13 x S (both sides
    are fp64 evaluations of the same polynomial)."""
    import torch
    c = dg.random_case(np.random.default_rng(40 + N), 8, N, base)
    f = _torch_forward(torch, float(np.float32(c["dt"])))    # dt as the C-ABI's float carries it
    th = [torch.tensor(dg.f32(c[k]), dtype=torch.float64, requires_grad=True)
          for k in ("mass", "inertia", "r_feet", "xref")]
    Ad, Bd = f(*th)
    fa, fb = dg.forward(*dg.inputs(c))
    assert np.abs(Ad.detach().numpy() - fa).max() < 1e-14          # the restatement is the function
    assert np.abs(Bd.detach().numpy() - fb).max() < 1e-14
    loss = (Ad * torch.tensor(c["g_Ad"])).sum() + (Bd * torch.tensor(c["g_Bd"])).sum()
    gm, gi, gr, gx = (g.numpy() for g in torch.autograd.grad(loss, th))
    vals, S = dg.ref_vjp(*dg.inputs(c), c["g_Ad"], c["g_Bd"])
    assert np.all(gx[:, :, :5] == 0.0) and np.all(gx[:, :, 6:] == 0.0)
    got = dict(mass=gm, inertia=gi, r_feet=gr, yaw=gx[:, :, 5].sum(1))
    worst = dg.worst_ratio(got, vals, S, tol=1e-13)
    # every step's yaw entry carries g_yaw / N
    spread = np.abs(gx[:, :, 5] - (vals["yaw"] / N)[:, None]).max(1) / (1e-13 * S["yaw"])
    tan = [torch.tensor(dg.f32(c["d_" + k]), dtype=torch.float64)
           for k in ("mass", "inertia", "r_feet", "xref")]
    _, (dA, dB) = torch.autograd.functional.jvp(f, tuple(t.detach() for t in th), tuple(tan))
    jv, jS = dg.ref_jvp(*dg.inputs(c), *[c["d_" + k] for k in dg.JVP_TANGENTS])
    jworst = dg.worst_ratio(dict(Ad=dA.numpy(), Bd=dB.numpy()), jv, jS, tol=1e-13)
    print("N", N, "worst |ref - torch| / (1e-13 S): vjp", worst, "yaw spread", float(spread.max()),
          "jvp", jworst)
    assert all(np.all(s > 0.0) for s in S.values()) and all(np.all(s > 0.0) for s in jS.values())
    assert max(worst.values()) <= 1.0 and spread.max() <= 1.0 and max(jworst.values()) <= 1.0


@pytest.mark.parametrize("N", [1, 5, 16])
def test_adjoint_identity_of_the_references(base, N):
    """<g_Ad, d_Ad> + <g_Bd, d_Bd> = g_mass d_mass + <g_I, d_I> + <g_r, d_r> + g_yaw dyaw per
    robot, within 1e-13 x the sum of |factor| |factor| over both sides."""
    c = dg.random_case(np.random.default_rng(50 + N), 8, N, base)
    g, _ = dg.ref_vjp(*dg.inputs(c), c["g_Ad"], c["g_Bd"])
    d, _ = dg.ref_jvp(*dg.inputs(c), *[c["d_" + k] for k in dg.JVP_TANGENTS])
    dyaw = dg.f32(c["d_xref"])[:, :, 5].sum(1) / N
    pairs = [(c["g_Ad"], d["Ad"]), (c["g_Bd"], d["Bd"]), (g["mass"], dg.f32(c["d_mass"])),
             (g["inertia"], dg.f32(c["d_inertia"])), (g["r_feet"], dg.f32(c["d_r_feet"])),
             (g["yaw"], dyaw)]
    dot = [(x * y).reshape(8, -1).sum(1) for x, y in pairs]
    mag = sum((np.abs(x) * np.abs(y)).reshape(8, -1).sum(1) for x, y in pairs)
    ratio = np.abs(dot[0] + dot[1] - sum(dot[2:])) / (1e-13 * mag)
    print("N", N, "worst adjoint mismatch / (1e-13 sum|.||.|):", float(ratio.max()))
    assert np.all(mag > 0.0) and ratio.max() <= 1.0


def test_composition_equals_central_differences():
    """L = c . w*(Ad, Bd(r_feet)) on three instances of the config-2 fixture, faces read off its
    fp32 w: g_r_feet = ref_vjp(vjp_util.ref_dense's g_Ad, g_Bd) against a central difference of
    r_feet -> forward -> w* in float64 along four random directions d, within
    1e-6 x sum |g_i| |d_i|.  The step starts at 1e-5 m and is halved until halving it moves the
    difference by less than the bar."""
    from cmpc import SolverParams, synth
    params = SolverParams()
    N = params.N
    case = kkt_util.fixture_case(load_fixture("qp_cfg2.npz"), "", params)
    b = synth.make_config(2, B=len(case["w"]))          # the batch the fixture was drawn from
    m, I, r, xr = (dg.f32(b[k]) for k in ("m", "I_world", "r_legs", "xref"))
    dt = float(b["dt"])
    Ad, Bd = dg._forward64(m, I, r, xr, dt)
    assert np.abs(Ad - case["Ad"]).max() < 1e-6 and np.abs(Bd - case["Bd"]).max() < 1e-6
    rng = np.random.default_rng(60)
    worst = 0.0
    for i in (0, 21, 42):
        iv = kkt_util.instance_values(case, i, params)
        contact = case["contact"][i]
        faces = gain_util.classify(contact, case["w"][i], iv["mu"], iv["fz_min"])
        rest = [case[k][i].astype(np.float64) for k in ("gd", "x0", "xref")]
        tail = (contact, faces, iv["Q"], iv["R"], iv["mu"], iv["fz_min"])
        cvec = rng.standard_normal(24 * N)
        vals, _ = vjp_util.ref_dense(Ad[i], Bd[i], *rest, *tail, cvec)
        one = lambda a: a[i:i + 1]                                           # noqa: E731
        g, _ = dg.ref_vjp(one(m), one(I), one(r), one(xr), dt, vals["Ad"][None], vals["Bd"][None])
        g_r = g["r_feet"][0]

        def loss(rr):
            A1, B1 = dg._forward64(one(m), one(I), rr[None], one(xr), dt)
            return float(cvec @ vjp_util.w_star(A1[0], B1[0], *rest, *tail))

        def fd(d, h):
            return (loss(r[i] + h * d) - loss(r[i] - h * d)) / (2.0 * h)

        for _ in range(4):
            d = rng.standard_normal(r[i].shape)
            bar = 1e-6 * float(np.sum(np.abs(g_r) * np.abs(d)))
            h = 1e-5
            cur = fd(d, h)
            for _halvings in range(6):
                nxt = fd(d, 0.5 * h)
                moved, cur, h = abs(nxt - cur), nxt, 0.5 * h
                if moved < bar:
                    break
            assert moved < bar, (i, h, moved, bar)
            ratio = abs(cur - float(np.sum(g_r * d))) / bar
            worst = max(worst, ratio)
            print("instance", i, "step", h, "fd", cur, "g . d", float(np.sum(g_r * d)),
                  "ratio", ratio)
    print("worst |fd - g . d| / (1e-6 sum|g||d|):", worst)
    assert worst <= 1.0


def test_struct_layouts_match_header(tmp_path):
    """sizeof / offsetof of cmpc_dynamics_vjp_io and cmpc_dynamics_jvp_io as a C compiler lays
    out include/cmpc.h; the ABI version did not move."""
    from cmpc import _lib
    from cmpc.build import hipcc
    structs = (("cmpc_dynamics_vjp_io", _lib.CDynamicsVjpIO), ("cmpc_dynamics_jvp_io", _lib.CDynamicsJvpIO))
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
    assert [n for n, _ in _lib.CDynamicsVjpIO._fields_] == [
        "size", "mass", "inertia", "r_feet", "xref", "dt", "g_Ad", "g_Bd", "g_mass", "g_inertia",
        "g_r_feet", "g_yaw"]
    assert [n for n, _ in _lib.CDynamicsJvpIO._fields_] == [
        "size", "mass", "inertia", "r_feet", "xref", "dt", "d_mass", "d_inertia", "d_r_feet",
        "d_xref", "d_Ad", "d_Bd"]
    assert _lib.DYNAMICS_VJP_OUTPUTS == dg.VJP_OUTPUTS
    assert _lib.DYNAMICS_JVP_TANGENTS == dg.JVP_TANGENTS


def test_argument_checks_that_need_no_plan():
    """A null io and a size that does not reach the first output are refused before the plan is
    touched; the entries are declared and exported."""
    from cmpc import _lib
    from cmpc.build import build_library, LIB
    from test_cabi import declared_symbols
    if not LIB.exists():
        build_library()
    lib = _lib.load()
    for entry, mirror, first in (("cmpc_dynamics_vjp_run", _lib.CDynamicsVjpIO, "g_mass"),
                                 ("cmpc_dynamics_jvp_run", _lib.CDynamicsJvpIO, "d_Ad")):
        assert entry in declared_symbols() and entry in _lib.EXPORTS and hasattr(lib, entry)
        fn = getattr(lib, entry)
        assert fn(None, 1, None, None) == -22 and "null io" in _lib.last_error(lib)
        io = mirror()
        io.size = getattr(mirror, first).offset          # ends just before the first output
        assert fn(None, 1, ctypes.byref(io), None) == -22
        assert "size" in _lib.last_error(lib) and entry in _lib.last_error(lib)
        io.size = ctypes.sizeof(mirror)
        assert fn(None, 1, ctypes.byref(io), None) == -22 and "null plan" in _lib.last_error(lib)
