"""CPU: the host side of cmpc_jvp_run (include/cmpc.h) -- the cmpc_jvp_io struct against its
ctypes mirror, the entry's export and argument checks -- and the test infrastructure of
tests/test_gpu_jvp.py: the two float64 references of jvp_util agree with each other, reference
(a) agrees with central differences of vjp_util.w_star along random directions, and with
vjp_util.ref_dense through the adjoint identity gw . dw = sum_theta g_theta . d_theta."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from parity_util import load_fixture
import gain_util
import jvp_util
import kkt_util
import vjp_util
from test_vjp import _random_problem, _consistent_faces

REQUIRED = ("Ad", "Bd", "gd", "x0", "xref", "contact", "dw")
FAKE = 64   # a non-null pointer value that is never dereferenced: the checks come first
IN = ("Ad", "Bd", "gd", "x0", "xref")
ALL = jvp_util.TANGENTS


@pytest.fixture(scope="module")
def lib():
    from cmpc import _lib
    from cmpc.build import build_library, LIB
    if not LIB.exists():
        build_library()
    return _lib.load()


def _io(**fields):
    from cmpc import _lib
    io = _lib.CJvpIO()
    io.size = ctypes.sizeof(_lib.CJvpIO)
    for k in REQUIRED + ("w", "d_x0"):
        setattr(io, k, FAKE)
    for k, v in fields.items():
        setattr(io, k, v)
    return io


def _refused(lib, plan, io, B=1):
    from cmpc import _lib
    rc = lib.cmpc_jvp_run(plan, B, None if io is None else ctypes.byref(io), None)
    msg = _lib.last_error(lib)
    assert rc == -22 and "cmpc_jvp_run" in msg, (rc, msg)
    return msg


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of cmpc_jvp_io as a C compiler lays out include/cmpc.h; the ABI version
    and the neighbouring structs did not move."""
    from cmpc import _lib
    from cmpc.build import hipcc
    names = [n for n, _ in _lib.CJvpIO._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cmpc.h"\nint main(void) {\n'
                   '  printf("%d\\n", CMPC_ABI_VERSION);\n'
                   '  printf("%zu\\n", sizeof(cmpc_jvp_io));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(cmpc_jvp_io, {n}));\n' for n in names) +
                   '  printf("%zu %zu %zu %zu\\n", sizeof(cmpc_params), sizeof(cmpc_kkt_io), '
                   'sizeof(cmpc_gain_io), sizeof(cmpc_vjp_io));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    cc = shutil.which("cc") or shutil.which("gcc")
    cmd = [cc, str(src)] if cc else [hipcc(), "-x", "c", str(src)]
    subprocess.run(cmd + [f"-I{REPO / 'include'}", "-o", str(exe)], check=True, timeout=120)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True,
                                           timeout=60).stdout.split()]
    assert vals[0] == 6 == _lib.ABI_VERSION
    assert vals[1] == ctypes.sizeof(_lib.CJvpIO)
    assert vals[2:-4] == [getattr(_lib.CJvpIO, n).offset for n in names]
    assert vals[-4:] == [176, ctypes.sizeof(_lib.CKktIO), ctypes.sizeof(_lib.CGainIO),
                         ctypes.sizeof(_lib.CVjpIO)]
    assert names == ["size", "Ad", "Bd", "gd", "x0", "xref", "contact", "mu", "fz_min", "Q", "R",
                     "w", "faces", "face_tol"] + ["d_" + n for n in ALL] + ["dw"]
    assert _lib.JVP_TANGENTS == ALL


def test_entry_is_declared_and_exported(lib):
    from cmpc import _lib, Plan
    from test_cabi import declared_symbols
    assert "cmpc_jvp_run" in declared_symbols()
    assert "cmpc_jvp_run" in _lib.EXPORTS and hasattr(lib, "cmpc_jvp_run")
    assert set(_lib.EXPORTS) == set(declared_symbols())
    assert callable(Plan.jvp)


def test_argument_checks_come_before_the_plan(lib):
    from cmpc import _lib
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert "null io" in _refused(lib, None, None)
    assert "null io" in _refused(lib, FAKE, None)
    # size must reach past dw (a FAKE plan: refused before the plan is read)
    short = _io()
    short.size = _lib.CJvpIO.dw.offset
    assert "size" in _refused(lib, FAKE, short)
    short.size = 4
    assert "size" in _refused(lib, FAKE, short)
    assert "null plan" in _refused(lib, None, _io())
    for name in REQUIRED:
        assert "null array" in _refused(lib, FAKE, _io(**{name: None})), name
    assert "both null" in _refused(lib, FAKE, _io(w=None, faces=None))
    # at least one tangent; any one of them will do
    assert "every tangent is null" in _refused(lib, FAKE, _io(d_x0=None))
    for n in ALL[1:]:
        assert "face_tol" in _refused(lib, FAKE, _io(d_x0=None, face_tol=-1.0, **{"d_" + n: FAKE})), n
    # a struct that ends right after dw is whole: it gets as far as the checks past the arrays
    ends = _io(face_tol=-1.0)
    ends.size = _lib.CJvpIO.dw.offset + ptr
    assert "face_tol" in _refused(lib, FAKE, ends)
    for tol in (-1e-6, float("nan"), float("inf"), -float("inf")):
        assert "face_tol" in _refused(lib, FAKE, _io(face_tol=tol)), tol
        assert "face_tol" in _refused(lib, FAKE, _io(face_tol=tol, w=None, faces=FAKE)), tol
    assert "B must be" in _refused(lib, FAKE, _io(), B=0)
    assert "B must be" in _refused(lib, FAKE, _io(w=None, faces=FAKE), B=-3)


def _args(c, i):
    return ([c[k][i] for k in IN + ("contact",)],
            dict(Q=c["Q"][i], R=c["R"][i], mu=float(c["mu"][i]), fz_min=float(c["fz_min"][i])))


def _theta(args, kw):
    return jvp_util.theta_of(*args[:5], kw["Q"], kw["R"], kw["mu"], kw["fz_min"])


def _agree(args, faces, kw, tangents, worst):
    """(a) against (b) at vjp_util.TOL_REFS, the zero rule on both -> (a)."""
    a = jvp_util.ref_dense(*args, faces, tangents=tangents, **kw)
    b, info = jvp_util.ref_riccati(*args, faces, tangents=tangents, **kw)
    S_x, S_u = jvp_util.scales(args[0], args[1], a, info)
    for j, r in enumerate(jvp_util.worst_ratio(b, a, S_x, S_u, vjp_util.TOL_REFS)):
        worst[j] = max(worst[j], r)
    N = args[1].shape[0]
    zero = jvp_util.zero_rule(args[5], faces).ravel()
    assert np.all(a[12 * N:][zero] == 0.0) and np.all(b[12 * N:][zero] == 0.0)
    return a


def test_the_assembly_difference_is_exact():
    """Every entry of the KKT matrix and right-hand side is a polynomial of degree <= 2 in theta:
    its central difference does not depend on the step."""
    rng = np.random.default_rng(5)
    c = _random_problem(rng, 3, B=1)
    faces = _consistent_faces(rng, c, 3)[0]
    args, kw = _args(c, 0)
    th = _theta(args, kw)
    t = jvp_util.random_tangents(rng, th)
    K1, r1 = jvp_util.kkt_derivative(th, t, args[5], faces, 1.0)
    K2, r2 = jvp_util.kkt_derivative(th, t, args[5], faces, 0.5)
    assert np.abs(K1).max() > 0.1 and np.abs(r1).max() > 0.1
    assert np.allclose(K1, K2, rtol=0.0, atol=1e-13 * max(1.0, np.abs(K1).max()))
    assert np.allclose(r1, r2, rtol=0.0, atol=1e-13 * max(1.0, np.abs(r1).max()))


@pytest.mark.parametrize("name,tag", kkt_util.FIXTURES)
def test_references_agree_on_the_fixtures(name, tag):
    """Reference (a) and (b) on every eighth instance of the fixture set, faces read off the
    fp32-rounded w, all nine tangents random: within 1e-9 x S."""
    from cmpc import SolverParams
    params = SolverParams()
    case = kkt_util.fixture_case(load_fixture(name), tag, params)
    rng = np.random.default_rng(11)
    worst = [0.0, 0.0]
    for i in range(0, len(case["w"]), 8):
        iv = kkt_util.instance_values(case, i, params)
        args, kw = gain_util.instance_args(case, i, iv)
        faces = gain_util.classify(case["contact"][i], case["w"][i], iv["mu"], iv["fz_min"])
        a = _agree(args, faces, kw, jvp_util.random_tangents(rng, _theta(args, kw)), worst)
        assert np.all(np.isfinite(a))
    print(name, tag, "worst |riccati - dense| / (1e-9 S): states, forces", worst)
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize("N", [1, 5])
def test_references_agree_on_random_problems(N):
    rng = np.random.default_rng(100 + N)
    c = _random_problem(rng, N, B=12)
    c["fz_min"][::4] = 0.0
    faces = _consistent_faces(rng, c, N)
    worst = [0.0, 0.0]
    for i in range(len(faces)):
        args, kw = _args(c, i)
        th = _theta(args, kw)
        _agree(args, faces[i], kw, jvp_util.random_tangents(rng, th), worst)
        n = ALL[i % 9]                                    # and one tangent alone
        _agree(args, faces[i], kw, jvp_util.random_tangents(rng, th, (n,)), worst)
    print("N", N, "worst |riccati - dense| / (1e-9 S): states, forces", worst)
    assert max(worst) <= 1.0, worst


def _fd(args, kw, faces, tangents, h=1e-5):
    th = _theta(args, kw)
    ws = []
    for sgn in (1.0, -1.0):
        t = jvp_util.moved(th, tangents, sgn * h)
        ws.append(vjp_util.w_star(*[t[k] for k in IN], args[5], faces, t["Q"], t["R"], t["mu"],
                                  t["fz_min"]))
    return (ws[0] - ws[1]) / (2.0 * h)


def _fd_check(args, kw, faces, tangents, worst, key):
    a = jvp_util.ref_dense(*args, faces, tangents=tangents, **kw)
    fd = _fd(args, kw, faces, tangents)
    worst[key] = max(worst.get(key, 0.0),
                     float(np.max(np.abs(fd - a)) / (1e-5 * max(1.0, np.abs(a).max()))))


@pytest.mark.parametrize("N", [1, 3])
def test_dense_reference_equals_central_differences(N):
    """|fd - (a)| <= 1e-5 x max(1, max|dw|) along random directions: each of the nine inputs
    alone and all nine together, on random problems and face sets."""
    rng = np.random.default_rng(200 + N)
    c = _random_problem(rng, N, B=3)
    c["fz_min"][1] = 0.0
    faces = _consistent_faces(rng, c, N)
    worst = {}
    for i in range(len(faces)):
        args, kw = _args(c, i)
        th = _theta(args, kw)
        for n in ALL:
            _fd_check(args, kw, faces[i], jvp_util.random_tangents(rng, th, (n,)), worst, n)
        _fd_check(args, kw, faces[i], jvp_util.random_tangents(rng, th), worst, "all")
    print("N", N, "worst |fd - dense| / (1e-5 max(1, max|dw|)):", worst)
    assert set(worst) == set(ALL) | {"all"} and max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("fz_min", [0.0, 7.5])
def test_central_differences_on_all_masks_of_one_leg(fz_min):
    """One stance leg, one step, every one of the 32 masks (the inconsistent ones are skipped:
    the entry answers NaN there), all nine tangents: a both-sign leg stays pinned at 0 whatever
    d_mu and d_fz_min are."""
    rng = np.random.default_rng(300)
    c = _random_problem(rng, 1, B=1)
    c["fz_min"][0] = np.float32(fz_min)
    c["contact"][0] = 0
    c["contact"][0, 2, 0] = 1
    args, kw = _args(c, 0)
    worst, done = {}, 0
    for mask in range(32):
        faces = np.zeros((1, 4), np.uint8)
        faces[0, 2] = mask
        if not gain_util.consistent(faces, c["contact"][0], float(c["mu"][0]), fz_min):
            continue
        t = jvp_util.random_tangents(rng, _theta(args, kw))
        _fd_check(args, kw, faces, t, worst, "all")
        _agree(args, faces, kw, t, [0.0, 0.0])
        done += 1
    assert done == (32 if fz_min == 0.0 else 25)
    print("fz_min", fz_min, "worst |fd - dense| / (1e-5 max(1, max|dw|)):", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("N", [1, 3])
def test_adjoint_identity_against_the_vjp_reference(N):
    """gw . dw = sum_theta g_theta . d_theta with vjp_util.ref_dense's gradients: the same
    Jacobian from both sides.  Tolerance: each side within its references' bar, 1e-9 x
    (sum |gw| S_w + sum_theta S_theta |d_theta|_1)."""
    rng = np.random.default_rng(400 + N)
    c = _random_problem(rng, N, B=4)
    c["fz_min"][2] = 0.0
    faces = _consistent_faces(rng, c, N)
    worst = 0.0
    for i in range(len(faces)):
        args, kw = _args(c, i)
        t = jvp_util.random_tangents(rng, _theta(args, kw))
        gw = vjp_util.random_gw(rng, 24 * N)
        dw = jvp_util.ref_dense(*args, faces[i], tangents=t, **kw)
        _, info = jvp_util.ref_riccati(*args, faces[i], tangents=t, **kw)
        S_x, S_u = jvp_util.scales(args[0], args[1], dw, info)
        g, S = vjp_util.ref_dense(*args, faces[i], gw=gw, **kw)
        lhs = float(gw.astype(np.float64) @ dw)
        rhs = sum(float(np.sum(g[n] * t[n].astype(np.float64))) for n in ALL)
        a = np.abs(gw.astype(np.float64))
        tol = vjp_util.TOL_REFS * (S_x * a[:12 * N].sum() + S_u * a[12 * N:].sum() +
                                   sum(S[n] * float(np.abs(t[n]).sum()) for n in ALL))
        assert abs(lhs) > 0.0
        worst = max(worst, abs(lhs - rhs) / tol)
    print("N", N, "worst |gw . dw - sum g . d| / tol:", worst)
    assert worst <= 1.0
