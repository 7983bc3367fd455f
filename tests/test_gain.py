"""CPU: the host side of cmpc_gain_run (include/cmpc.h) -- the cmpc_gain_io struct against its
ctypes mirror, the entry's export and argument checks -- and the test infrastructure of
tests/test_gpu_gain.py: the two float64 references of gain_util agree with each other, and the
mask rule of a leg's affine set agrees with the SVD of its face rows."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from parity_util import load_fixture
import gain_util
import kkt_util

REQUIRED = ("Ad", "Bd", "gd", "x0", "xref", "contact", "K")
FAKE = 64   # a non-null pointer value that is never dereferenced: the checks come first


@pytest.fixture(scope="module")
def lib():
    from cmpc import _lib
    from cmpc.build import build_library, LIB
    if not LIB.exists():
        build_library()
    return _lib.load()


def _io(**fields):
    from cmpc import _lib
    io = _lib.CGainIO()
    io.size = ctypes.sizeof(_lib.CGainIO)
    for k in REQUIRED + ("w",):
        setattr(io, k, FAKE)
    for k, v in fields.items():
        setattr(io, k, v)
    return io


def _refused(lib, plan, io, B=1):
    from cmpc import _lib
    rc = lib.cmpc_gain_run(plan, B, None if io is None else ctypes.byref(io), None)
    msg = _lib.last_error(lib)
    assert rc == -22 and "cmpc_gain_run" in msg, (rc, msg)
    return msg


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of cmpc_gain_io as a C compiler lays out include/cmpc.h, the face bits
    and the ABI version the header prints."""
    from cmpc import _lib
    from cmpc.build import hipcc
    names = [n for n, _ in _lib.CGainIO._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cmpc.h"\nint main(void) {\n'
                   '  printf("%d\\n", CMPC_ABI_VERSION);\n'
                   '  printf("%zu\\n", sizeof(cmpc_gain_io));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(cmpc_gain_io, {n}));\n' for n in names) +
                   '  printf("%d %d %d %d %d\\n", CMPC_FACE_FZ_MIN, CMPC_FACE_FX_POS, '
                   'CMPC_FACE_FX_NEG, CMPC_FACE_FY_POS, CMPC_FACE_FY_NEG);\n'
                   '  printf("%zu %zu\\n", sizeof(cmpc_params), sizeof(cmpc_kkt_io));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    cc = shutil.which("cc") or shutil.which("gcc")
    cmd = [cc, str(src)] if cc else [hipcc(), "-x", "c", str(src)]
    subprocess.run(cmd + [f"-I{REPO / 'include'}", "-o", str(exe)], check=True, timeout=120)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True,
                                           timeout=60).stdout.split()]
    assert vals[0] == 6 == _lib.ABI_VERSION
    assert vals[1] == ctypes.sizeof(_lib.CGainIO)
    assert vals[2:-7] == [getattr(_lib.CGainIO, n).offset for n in names]
    assert vals[-7:-2] == [1, 2, 4, 8, 16] == [_lib.FACE_FZ_MIN, _lib.FACE_FX_POS, _lib.FACE_FX_NEG,
                                               _lib.FACE_FY_POS, _lib.FACE_FY_NEG]
    assert vals[-2:] == [176, ctypes.sizeof(_lib.CKktIO)]       # the neighbours did not move
    assert names == ["size", "Ad", "Bd", "gd", "x0", "xref", "contact", "mu", "fz_min", "Q", "R",
                     "w", "faces", "face_tol", "K", "Vx", "Vxx", "u_star", "faces_out"]
    assert [gain_util.FZ_MIN, gain_util.FX_POS, gain_util.FX_NEG, gain_util.FY_POS,
            gain_util.FY_NEG] == [1, 2, 4, 8, 16]


def test_entry_is_declared_and_exported(lib):
    from cmpc import _lib, Plan
    from test_cabi import declared_symbols
    assert "cmpc_gain_run" in declared_symbols()
    assert "cmpc_gain_run" in _lib.EXPORTS and hasattr(lib, "cmpc_gain_run")
    assert callable(Plan.gain)


def test_argument_checks_come_before_the_plan(lib):
    from cmpc import _lib
    assert "null io" in _refused(lib, None, None)
    assert "null io" in _refused(lib, FAKE, None)
    # size must reach past K (a FAKE plan: refused before the plan is read)
    short = _io()
    short.size = _lib.CGainIO.K.offset
    assert "size" in _refused(lib, FAKE, short)
    short.size = 4
    assert "size" in _refused(lib, FAKE, short)
    assert "null plan" in _refused(lib, None, _io())
    for name in REQUIRED:
        assert "null array" in _refused(lib, FAKE, _io(**{name: None})), name
    assert "both null" in _refused(lib, FAKE, _io(w=None, faces=None))
    # a struct that ends after K reads the outputs past it as NULL, and still needs w or faces
    ends = _io(w=None, faces=None)
    ends.size = _lib.CGainIO.K.offset + ctypes.sizeof(ctypes.c_void_p)
    assert "both null" in _refused(lib, FAKE, ends)
    for tol in (-1e-6, float("nan"), float("inf"), -float("inf")):
        assert "face_tol" in _refused(lib, FAKE, _io(face_tol=tol)), tol
        assert "face_tol" in _refused(lib, FAKE, _io(face_tol=tol, w=None, faces=FAKE)), tol
    assert "B must be" in _refused(lib, FAKE, _io(), B=0)
    assert "B must be" in _refused(lib, FAKE, _io(w=None, faces=FAKE), B=-3)


@pytest.mark.parametrize("name,tag", kkt_util.FIXTURES)
def test_references_agree_on_the_fixtures(name, tag):
    """Reference (a), the dense KKT solve, and (b), the Riccati recursion, on every eighth
    instance of the fixture set, faces read off the fp32-rounded w: within 1e-9 x scale."""
    from cmpc import SolverParams
    params = SolverParams()
    case = kkt_util.fixture_case(load_fixture(name), tag, params)
    worst = {n: 0.0 for n in gain_util.OUTPUTS}
    free = []
    for i in range(0, len(case["w"]), 8):
        iv = kkt_util.instance_values(case, i, params)
        args, kw = gain_util.instance_args(case, i, iv)
        faces = gain_util.classify(case["contact"][i], case["w"][i], iv["mu"], iv["fz_min"])
        assert gain_util.consistent(faces, case["contact"][i], iv["mu"], iv["fz_min"])
        vals, S = gain_util.ref_dense(*args, faces, **kw)
        ric = gain_util.ref_riccati(*args, faces, **kw)
        for n, r in gain_util.worst_ratio(ric, vals, S, tol=1e-9).items():
            worst[n] = max(worst[n], r)
        free.append(sum(gain_util.leg_set_svd(int(faces[k, leg]), iv["mu"], iv["fz_min"])[0].shape[1]
                        for k in range(faces.shape[0]) for leg in range(4)
                        if case["contact"][i][leg, k]))
        # the optimum on the held faces is the fixture's optimum, to the fp32 rounding of w
        U = case["w"][i][12 * faces.shape[0]:].astype(np.float64)
        assert np.max(np.abs(vals["u_star"] - U)) <= 1e-5 * max(1.0, np.abs(U).max())
        assert np.all(np.isfinite(vals["K"]))
    print(name, tag, "free force parameters", min(free), "..", max(free),
          "worst |riccati - dense| / (1e-9 scale):", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("fz_min", [0.0, 10.0])
def test_mask_rule_equals_the_svd_of_the_face_rows(fz_min):
    """All 32 masks: the affine set of the mask rule (what the kernel builds) is the solution set
    of the mask's face rows, and exactly the inconsistent masks are flagged."""
    mu = 0.6
    flagged = []
    for mask in range(32):
        Zs, cs, ok_s = gain_util.leg_set_svd(mask, mu, fz_min)
        Zr, cr, ok_r = gain_util.leg_set_rule(mask, mu, fz_min)
        assert ok_s == ok_r, mask
        if not ok_r:
            flagged.append(mask)
            continue
        A, b = gain_util.leg_rows(mask, mu, fz_min)
        assert Zr.shape == Zs.shape, mask                        # the same dimension
        if len(A):
            assert np.allclose(A @ cr, b, rtol=0, atol=1e-12), mask      # c is on every face
            assert np.allclose(A @ Zr, 0.0, rtol=0, atol=1e-12), mask    # Z spans their null space
        assert Zr.shape[1] == 0 or np.linalg.matrix_rank(Zr) == Zr.shape[1], mask
        # and the two sets are one: the SVD's point lies in the rule's set
        resid = (cs - cr) - Zr @ np.linalg.lstsq(Zr, cs - cr, rcond=None)[0] if Zr.shape[1] else cs - cr
        assert np.allclose(resid, 0.0, rtol=0, atol=1e-12), mask
    both = [m for m in range(32) if (m & 6) == 6 or (m & 24) == 24]
    want = [m for m in both if m & 1] if fz_min != 0.0 else []
    assert flagged == want
