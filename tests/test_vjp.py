"""CPU: the host side of cmpc_vjp_run (include/cmpc.h) -- the cmpc_vjp_io struct against its
ctypes mirror, the entry's export and argument checks -- and the test infrastructure of
tests/test_gpu_vjp.py: the two float64 references of vjp_util agree with each other, and
reference (a) agrees with central differences of gw . w*(theta) in every entry of every input."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from parity_util import load_fixture
import gain_util
import kkt_util
import vjp_util

REQUIRED = ("Ad", "Bd", "gd", "x0", "xref", "contact", "gw")
FAKE = 64   # a non-null pointer value that is never dereferenced: the checks come first
IN = ("Ad", "Bd", "gd", "x0", "xref")


@pytest.fixture(scope="module")
def lib():
    from cmpc import _lib
    from cmpc.build import build_library, LIB
    if not LIB.exists():
        build_library()
    return _lib.load()


def _io(**fields):
    from cmpc import _lib
    io = _lib.CVjpIO()
    io.size = ctypes.sizeof(_lib.CVjpIO)
    for k in REQUIRED + ("w", "g_x0"):
        setattr(io, k, FAKE)
    for k, v in fields.items():
        setattr(io, k, v)
    return io


def _refused(lib, plan, io, B=1):
    from cmpc import _lib
    rc = lib.cmpc_vjp_run(plan, B, None if io is None else ctypes.byref(io), None)
    msg = _lib.last_error(lib)
    assert rc == -22 and "cmpc_vjp_run" in msg, (rc, msg)
    return msg


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of cmpc_vjp_io as a C compiler lays out include/cmpc.h; the ABI version
    and the neighbouring structs did not move."""
    from cmpc import _lib
    from cmpc.build import hipcc
    names = [n for n, _ in _lib.CVjpIO._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cmpc.h"\nint main(void) {\n'
                   '  printf("%d\\n", CMPC_ABI_VERSION);\n'
                   '  printf("%zu\\n", sizeof(cmpc_vjp_io));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(cmpc_vjp_io, {n}));\n' for n in names) +
                   '  printf("%zu %zu %zu\\n", sizeof(cmpc_params), sizeof(cmpc_kkt_io), '
                   'sizeof(cmpc_gain_io));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    cc = shutil.which("cc") or shutil.which("gcc")
    cmd = [cc, str(src)] if cc else [hipcc(), "-x", "c", str(src)]
    subprocess.run(cmd + [f"-I{REPO / 'include'}", "-o", str(exe)], check=True, timeout=120)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True,
                                           timeout=60).stdout.split()]
    assert vals[0] == 6 == _lib.ABI_VERSION
    assert vals[1] == ctypes.sizeof(_lib.CVjpIO)
    assert vals[2:-3] == [getattr(_lib.CVjpIO, n).offset for n in names]
    assert vals[-3:] == [176, ctypes.sizeof(_lib.CKktIO), ctypes.sizeof(_lib.CGainIO)]
    assert names == ["size", "Ad", "Bd", "gd", "x0", "xref", "contact", "mu", "fz_min", "Q", "R",
                     "w", "faces", "face_tol", "gw"] + ["g_" + n for n in vjp_util.OUTPUTS]
    assert _lib.VJP_OUTPUTS == vjp_util.OUTPUTS


def test_entry_is_declared_and_exported(lib):
    from cmpc import _lib, Plan, autograd
    from test_cabi import declared_symbols
    assert "cmpc_vjp_run" in declared_symbols()
    assert "cmpc_vjp_run" in _lib.EXPORTS and hasattr(lib, "cmpc_vjp_run")
    assert callable(Plan.vjp) and callable(autograd.solve)


def test_argument_checks_come_before_the_plan(lib):
    from cmpc import _lib
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert "null io" in _refused(lib, None, None)
    assert "null io" in _refused(lib, FAKE, None)
    # size must reach past g_x0 (a FAKE plan: refused before the plan is read)
    short = _io()
    short.size = _lib.CVjpIO.g_x0.offset
    assert "size" in _refused(lib, FAKE, short)
    short.size = 4
    assert "size" in _refused(lib, FAKE, short)
    assert "null plan" in _refused(lib, None, _io())
    for name in REQUIRED:
        assert "null array" in _refused(lib, FAKE, _io(**{name: None})), name
    assert "both null" in _refused(lib, FAKE, _io(w=None, faces=None))
    # at least one output; any one of them will do
    assert "every output is null" in _refused(lib, FAKE, _io(g_x0=None))
    for n in vjp_util.OUTPUTS[1:]:
        assert "face_tol" in _refused(lib, FAKE, _io(g_x0=None, face_tol=-1.0, **{"g_" + n: FAKE})), n
    # a struct that ends after g_x0 reads the outputs past it as NULL
    ends = _io(g_x0=None, g_Bd=FAKE)
    ends.size = _lib.CVjpIO.g_x0.offset + ptr
    assert "every output is null" in _refused(lib, FAKE, ends)
    ends = _io(w=None, faces=None)
    ends.size = _lib.CVjpIO.g_x0.offset + ptr
    assert "both null" in _refused(lib, FAKE, ends)
    for tol in (-1e-6, float("nan"), float("inf"), -float("inf")):
        assert "face_tol" in _refused(lib, FAKE, _io(face_tol=tol)), tol
        assert "face_tol" in _refused(lib, FAKE, _io(face_tol=tol, w=None, faces=FAKE)), tol
    assert "B must be" in _refused(lib, FAKE, _io(), B=0)
    assert "B must be" in _refused(lib, FAKE, _io(w=None, faces=FAKE), B=-3)


def _agree(args, faces, kw, gw, worst):
    va, Sa = vjp_util.ref_dense(*args, faces, gw=gw, **kw)
    vb, Sb = vjp_util.ref_riccati(*args, faces, gw=gw, **kw)
    for n, r in vjp_util.worst_ratio(vb, va, Sa, vjp_util.TOL_REFS).items():
        worst[n] = max(worst[n], r)
        assert (Sa[n] == 0.0) == (Sb[n] == 0.0), n      # the same structural zeros
    return va


@pytest.mark.parametrize("name,tag", kkt_util.FIXTURES)
def test_references_agree_on_the_fixtures(name, tag):
    """Reference (a), the dense KKT solve, and (b), the kernel's route in NumPy, on every eighth
    instance of the fixture set, faces read off the fp32-rounded w, gw ~ N(0, 1) in fp32: within
    1e-9 x S per output."""
    from cmpc import SolverParams
    params = SolverParams()
    case = kkt_util.fixture_case(load_fixture(name), tag, params)
    rng = np.random.default_rng(11)
    worst = {n: 0.0 for n in vjp_util.OUTPUTS}
    for i in range(0, len(case["w"]), 8):
        iv = kkt_util.instance_values(case, i, params)
        args, kw = gain_util.instance_args(case, i, iv)
        faces = gain_util.classify(case["contact"][i], case["w"][i], iv["mu"], iv["fz_min"])
        va = _agree(args, faces, kw, vjp_util.random_gw(rng, case["w"][i].shape), worst)
        assert all(np.all(np.isfinite(v)) for v in va.values())
    print(name, tag, "worst |riccati - dense| / (1e-9 S):", worst)
    assert max(worst.values()) <= 1.0, worst


def _random_problem(rng, N, B=1):
    """test_gpu_gain.random_case's distributions without its special instances."""
    c = dict(Ad=np.eye(12) + 0.05 * rng.standard_normal((B, 12, 12)),
             Bd=0.1 * rng.standard_normal((B, N, 12, 12)), gd=0.1 * rng.standard_normal((B, 12)),
             x0=rng.standard_normal((B, 12)), xref=rng.standard_normal((B, N, 12)),
             mu=rng.uniform(0.2, 1.0, B), fz_min=rng.uniform(1.0, 20.0, B),
             Q=rng.uniform(0.0, 50.0, (B, 12)), R=rng.uniform(1e-4, 1e-2, (B, 12)))
    c = {k: kkt_util.f32(v) for k, v in c.items()}
    c["contact"] = (rng.random((B, 4, N)) < 0.7).astype(np.uint8)
    return c


def _consistent_faces(rng, c, N):
    faces = rng.integers(0, 32, (len(c["Ad"]), N, 4)).astype(np.uint8)
    faces[rng.random(faces.shape) < 0.35] = 0
    both = ((faces & 6) == 6) | ((faces & 24) == 24)
    faces[both & ((faces & 1) != 0) & (c["fz_min"] != 0)[:, None, None]] &= 0xFE
    return faces


@pytest.mark.parametrize("N", [1, 5])
def test_references_agree_on_random_problems(N):
    rng = np.random.default_rng(100 + N)
    c = _random_problem(rng, N, B=12)
    c["fz_min"][::4] = 0.0
    faces = _consistent_faces(rng, c, N)
    worst = {n: 0.0 for n in vjp_util.OUTPUTS}
    for i in range(len(faces)):
        args = [c[k][i] for k in IN + ("contact",)]
        kw = dict(Q=c["Q"][i], R=c["R"][i], mu=float(c["mu"][i]), fz_min=float(c["fz_min"][i]))
        _agree(args, faces[i], kw, vjp_util.random_gw(rng, 24 * N), worst)
    print("N", N, "worst |riccati - dense| / (1e-9 S):", worst)
    assert max(worst.values()) <= 1.0, worst


def _central_differences(th, contact, faces, gw):
    """d (gw . w*(theta)) / d theta in every entry of every input: step 1e-5 x max(1, |theta|),
    for R 1e-4 x R."""
    gw = gw.astype(np.float64)

    def loss(t):
        return float(gw @ vjp_util.w_star(*[t[k] for k in IN], contact, faces, t["Q"], t["R"],
                                          t["mu"], t["fz_min"]))
    out = {}
    for n in vjp_util.OUTPUTS:
        base = np.asarray(th[n], np.float64)
        g = np.zeros(base.shape)
        for idx in (np.ndindex(*base.shape) if base.shape else [()]):
            h = 1e-4 * abs(base[idx]) if n == "R" else 1e-5 * max(1.0, abs(base[idx]))
            vals = []
            for sgn in (1.0, -1.0):
                moved = base.copy()
                moved[idx] += sgn * h
                vals.append(loss(dict(th, **{n: moved})))
            g[idx] = (vals[0] - vals[1]) / (2.0 * h)
        out[n] = g
    return out


def _fd_check(c, i, faces, gw, worst):
    th = {k: c[k][i].astype(np.float64) for k in IN + ("Q", "R")}
    th["mu"], th["fz_min"] = np.float64(c["mu"][i]), np.float64(c["fz_min"][i])
    va, _ = vjp_util.ref_dense(*[th[k] for k in IN], c["contact"][i], faces, th["Q"], th["R"],
                               float(th["mu"]), float(th["fz_min"]), gw)
    fd = _central_differences(th, c["contact"][i], faces, gw)
    for n in vjp_util.OUTPUTS:
        r = float(np.max(np.abs(fd[n] - va[n])) / (1e-5 * max(1.0, np.abs(va[n]).max())))
        worst[n] = max(worst[n], r)


@pytest.mark.parametrize("N", [1, 3])
def test_dense_reference_equals_central_differences(N):
    """|fd - (a)| <= 1e-5 x max(1, max|that output|) on random problems and face sets."""
    rng = np.random.default_rng(200 + N)
    c = _random_problem(rng, N, B=3)
    c["fz_min"][1] = 0.0
    faces = _consistent_faces(rng, c, N)
    worst = {n: 0.0 for n in vjp_util.OUTPUTS}
    for i in range(len(faces)):
        _fd_check(c, i, faces[i], vjp_util.random_gw(rng, 24 * N), worst)
    print("N", N, "worst |fd - dense| / (1e-5 max(1, max|g|)):", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("fz_min", [0.0, 7.5])
def test_central_differences_on_all_masks_of_one_leg(fz_min):
    """One stance leg, one step, every one of the 32 masks (the inconsistent ones are skipped:
    the entry answers NaN there): both-sign masks, masks without a friction face, a pinned fz.
    A both-sign leg is pinned at fz = 0 whatever mu and fz_min are, so its rows keep a zero
    right-hand side under the differences too (vjp_util.face_rows)."""
    rng = np.random.default_rng(300)
    c = _random_problem(rng, 1, B=1)
    c["fz_min"][0] = np.float32(fz_min)
    c["contact"][0] = 0
    c["contact"][0, 2, 0] = 1
    worst = {n: 0.0 for n in vjp_util.OUTPUTS}
    done = 0
    for mask in range(32):
        faces = np.zeros((1, 4), np.uint8)
        faces[0, 2] = mask
        if not gain_util.consistent(faces, c["contact"][0], float(c["mu"][0]), fz_min):
            continue
        _fd_check(c, 0, faces, vjp_util.random_gw(rng, 24), worst)
        done += 1
    assert done == (32 if fz_min == 0.0 else 25)
    print("fz_min", fz_min, "worst |fd - dense| / (1e-5 max(1, max|g|)):", worst)
    assert max(worst.values()) <= 1.0, worst
