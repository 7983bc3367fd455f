"""CPU: the host side of cmpc_kkt_run (include/cmpc.h) -- the cmpc_kkt_io struct against its
ctypes mirror, the entry's export and argument checks, and the threshold guard that makes the
device-versus-NumPy comparison of recovered multipliers (tests/test_gpu_kkt.py) well defined."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from parity_util import load_fixture
import kkt_util

REQUIRED = ("Ad", "Bd", "gd", "x0", "xref", "contact", "w", "res")
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
    io = _lib.CKktIO()
    io.size = ctypes.sizeof(_lib.CKktIO)
    for k in REQUIRED:
        setattr(io, k, FAKE)
    for k, v in fields.items():
        setattr(io, k, v)
    return io


def _refused(lib, plan, io, B=1):
    from cmpc import _lib
    rc = lib.cmpc_kkt_run(plan, B, None if io is None else ctypes.byref(io), None)
    msg = _lib.last_error(lib)
    assert rc == -22 and "cmpc_kkt_run" in msg, (rc, msg)
    return msg


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of cmpc_kkt_io as a C compiler lays out include/cmpc.h, and the ABI
    version the header prints."""
    from cmpc import _lib
    from cmpc.build import hipcc
    names = [n for n, _ in _lib.CKktIO._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cmpc.h"\nint main(void) {\n'
                   '  printf("%d\\n", CMPC_ABI_VERSION);\n'
                   '  printf("%zu\\n", sizeof(cmpc_kkt_io));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(cmpc_kkt_io, {n}));\n' for n in names) +
                   '  printf("%d %d %d %d\\n", CMPC_KKT_COST, CMPC_KKT_STAT, CMPC_KKT_PRIM, '
                   'CMPC_KKT_COMP);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    cc = shutil.which("cc") or shutil.which("gcc")
    cmd = [cc, str(src)] if cc else [hipcc(), "-x", "c", str(src)]
    subprocess.run(cmd + [f"-I{REPO / 'include'}", "-o", str(exe)], check=True, timeout=120)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True,
                                           timeout=60).stdout.split()]
    assert vals[0] == 6 == _lib.ABI_VERSION
    assert vals[1] == ctypes.sizeof(_lib.CKktIO)
    assert vals[2:-4] == [getattr(_lib.CKktIO, n).offset for n in names]
    assert vals[-4:] == [0, 1, 2, 3]
    assert names[0] == "size" and names[-1] == "res"
    import cmpc
    assert cmpc.KKT_COLUMNS == ("cost", "stat", "prim", "comp")


def test_entry_is_declared_and_exported(lib):
    from cmpc import _lib
    from test_cabi import declared_symbols
    assert "cmpc_kkt_run" in declared_symbols()
    assert "cmpc_kkt_run" in _lib.EXPORTS and hasattr(lib, "cmpc_kkt_run")


def test_argument_checks_come_before_the_plan(lib):
    from cmpc import _lib
    assert "null io" in _refused(lib, None, None)
    assert "null io" in _refused(lib, FAKE, None)
    # size must reach past res (a FAKE plan: refused before the plan is read)
    short = _io()
    short.size = _lib.CKktIO.res.offset
    assert "size" in _refused(lib, FAKE, short)
    short.size = 4
    assert "size" in _refused(lib, FAKE, short)
    assert "null plan" in _refused(lib, None, _io())
    for name in REQUIRED:
        assert "null array" in _refused(lib, FAKE, _io(**{name: None})), name
    for tol in (-1e-6, float("nan"), float("inf"), -float("inf")):
        assert "face_tol" in _refused(lib, FAKE, _io(face_tol=tol)), tol
    assert "B must be" in _refused(lib, FAKE, _io(), B=0)


@pytest.mark.parametrize("name,tag", kkt_util.FIXTURES)
def test_no_held_face_test_sits_on_its_threshold(name, tag):
    """Threshold guard for test_gpu_kkt.py::test_fixtures_recovered_multipliers: on the
    fp32-rounded w of every fixture used there, no value duals.recover compares lies within a
    relative 1e-9 of its threshold, so rounding (an FMA contraction) cannot flip a face.  And the
    recovered multipliers of a sample have finite residuals (printed): no multiplier takes the
    sign of an infinite bound."""
    from cmpc import SolverParams
    params = SolverParams()
    case = kkt_util.fixture_case(load_fixture(name), tag, params)
    gap = np.inf
    for i in range(len(case["w"])):
        iv = kkt_util.instance_values(case, i, params)
        v, t = kkt_util.held_face_tests(case["contact"][i], case["w"][i], iv["mu"], iv["fz_min"])
        assert len(v) and np.all(t > 0)
        gap = min(gap, float(np.min(np.abs(v - t) / t)))
    print(name, tag, "smallest relative distance to a threshold", gap)
    assert gap > 1e-9
    vals, _ = kkt_util.case_ref(case, params, with_lam=False, idx=range(0, len(case["w"]), 8))
    print(name, tag, "recovered multipliers on the rounded optimum: stat, prim, comp <=",
          vals[:, 1:].max(axis=0))
    # (the fixture's optimum rounded to fp32: residuals of fp32 size, not 1e-8; no sign fault)
    assert np.all(np.isfinite(vals))
