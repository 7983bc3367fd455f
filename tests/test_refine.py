"""CPU: the NumPy model of the certified refinement (tests/refine_util.py, the reference of
tests/test_gpu_refine.py) on the committed fixtures and against oracle.active_set, and the host
side of cmpc_refine_run (include/cmpc.h): the cmpc_refine_io struct against its ctypes mirror,
the entry's export and its argument checks."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from parity_util import load_fixture
import kkt_util
import refine_util

SETS = ("qp_cfg1.npz", "qp_cfg2.npz", "qp_hard.npz", "qp_nc192.npz")
REQUIRED = ("Ad", "Bd", "gd", "x0", "xref", "contact", "info")
FAKE = 64   # a non-null pointer value that is never dereferenced: the checks come first
_cache = {}


def _params():
    from cmpc import SolverParams
    return SolverParams()


def _base(name):
    """(case, the model's results from the fp32 fixture w, max_rounds = 8), computed once."""
    if name not in _cache:
        case = kkt_util.fixture_case(load_fixture(name), "", _params())
        _cache[name] = (case, [refine_util.model_case(case, i, _params())
                               for i in range(len(case["w"]))])
    return _cache[name]


def _oracle_forces(name, i):
    """The certified optimum's forces of instance i and its result dict, computed once."""
    key = (name, "oracle", i)
    if key not in _cache:
        case = _base(name)[0]
        r = refine_util.oracle_optimum(case, i, _params(), case["w"][i])
        assert not r["fallback"] and max(r["kkt"].values()) <= 1e-8
        _cache[key] = r
    return _cache[key]


@pytest.mark.parametrize("name", SETS)
def test_model_certifies_the_fixtures(name):
    """From the fp32 fixture w every instance is certified: without a repair on qp_cfg1, qp_cfg2
    and qp_hard, with at most one on qp_nc192; res[2], the distance of the fp32 w from the
    float64 optimum, is fp32 rounding."""
    case, out = _base(name)
    info = np.array([o["info"] for o in out])
    print(name, "info", dict(zip(*np.unique(info, return_counts=True))), "max res[2]",
          max(o["res"][2] for o in out))
    assert np.all(info >= 0)
    assert np.all(info <= (1 if name == "qp_nc192.npz" else 0))
    assert all(o["res"][0] <= 1e-9 and o["res"][1] >= -1e-9 for o in out)
    assert max(o["res"][2] for o in out) <= 1e-5


@pytest.mark.parametrize("name", SETS)
def test_model_equals_the_oracle(name):
    """Every eighth instance (all four of qp_hard): the model's forces are the certified
    optimum's within 1e-10 x max|u|, and its multipliers with its point pass the oracle's
    certificate."""
    from oracle import active_set, mpc_qp
    case, out = _base(name)
    N = case["Bd"].shape[1]
    worst = 0.0
    for i in range(0, len(out), 8 if len(out) > 4 else 1):
        r = _oracle_forces(name, i)
        uo = r["w"][12 * N:]
        worst = max(worst, float(np.abs(out[i]["u"] - uo).max() / np.abs(uo).max()))
        w64 = np.concatenate([out[i]["x"].reshape(-1), out[i]["u"]])
        kkt = mpc_qp.kkt_residuals(r["qp"], w64, out[i]["lam"][:24 * N], out[i]["lam"][24 * N:])
        assert max(kkt.values()) <= active_set.CERT_TOL, (i, kkt)
    print(name, "worst |model - oracle| / max|u|:", worst)
    assert worst <= refine_util.ORACLE_REL


@pytest.mark.parametrize("name", ("qp_cfg2.npz", "qp_nc192.npz"))
@pytest.mark.parametrize("recipe", ("drop", "add"))
def test_model_repairs_one_wrong_face(name, recipe):
    """One held face dropped or one free face added per instance (default_rng(7)), max_rounds =
    8: every certified instance is the oracle's optimum, at most 2 of 64 are not certified, and
    those end in ROUNDS or CYCLE."""
    case, out = _base(name)
    N = case["Bd"].shape[1]
    f0 = np.stack([o["faces"] for o in out])
    seeds = refine_util.wrong_face_seeds(f0, case["contact"], recipe)
    # (an instance that holds no face has none to drop: 3 of qp_cfg2)
    assert np.sum(np.any(seeds != f0, axis=(1, 2))) >= len(f0) - 4
    assert np.all(np.sum(seeds != f0, axis=(1, 2)) <= 1)
    got = [refine_util.model_case(case, i, _params(), faces=seeds[i]) for i in range(len(f0))]
    info = np.array([o["info"] for o in got])
    print(name, recipe, "info", dict(zip(*np.unique(info, return_counts=True))))
    assert np.sum(info < 0) <= 2
    assert set(info[info < 0]) <= {refine_util.ROUNDS, refine_util.CYCLE}
    assert np.all(info <= 8)
    for i in np.flatnonzero(info >= 0):
        uo = _oracle_forces(name, i)["w"][12 * N:]
        assert np.abs(got[i]["u"] - uo).max() <= refine_util.ORACLE_REL * np.abs(uo).max(), i
    # what tests/test_gpu_refine.py relies on: fewer than 5 % of these instances have a decision
    # within a factor of 2 of its threshold, at every repair limit it uses
    unclear = {8: sum(o["margin"] < refine_util.CLEAR for o in got)}
    for rounds in (0, 2):
        few = [refine_util.model_case(case, i, _params(), faces=seeds[i], max_rounds=rounds)
               for i in range(len(f0))]
        unclear[rounds] = sum(o["margin"] < refine_util.CLEAR for o in few)
        # a lower limit stops the same sequence early: ROUNDS, or the same certified point
        for i, o in enumerate(few):
            if info[i] != refine_util.CYCLE:     # (a cycle may close before the lower limit)
                assert o["info"] == (info[i] if 0 <= info[i] <= rounds else refine_util.ROUNDS), i
        if rounds == 0:      # a check only: no mask is changed
            assert all(np.array_equal(o["faces"], np.where(case["contact"][i].T != 0, seeds[i], 0))
                       for i, o in enumerate(few))
    print("unclear instances per repair limit:", unclear)
    assert max(unclear.values()) < 0.05 * len(f0)


def test_model_flags_invalid_instances():
    case, out = _base("qp_cfg1.npz")
    faces = out[0]["faces"].copy()
    k, leg = np.argwhere(case["contact"][0].T != 0)[0]
    faces[k, leg] = 2 | 4
    o = refine_util.model_case(case, 0, _params(), faces=faces)
    assert o["info"] == refine_util.INVALID and np.all(o["faces"] == 0xFF)
    assert np.all(np.isnan(o["u"])) and np.all(np.isnan(o["lam"])) and np.all(np.isnan(o["res"]))


@pytest.fixture(scope="module")
def lib():
    from cmpc import _lib
    from cmpc.build import build_library, LIB
    if not LIB.exists():
        build_library()
    return _lib.load()


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of cmpc_refine_io as a C compiler lays out include/cmpc.h, and the
    info values."""
    from cmpc import _lib
    from cmpc.build import hipcc
    names = [n for n, _ in _lib.CRefineIO._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cmpc.h"\nint main(void) {\n'
                   '  printf("%d\\n", CMPC_ABI_VERSION);\n'
                   '  printf("%zu\\n", sizeof(cmpc_refine_io));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(cmpc_refine_io, {n}));\n' for n in names) +
                   '  printf("%d %d %d %d\\n", CMPC_REFINE_INVALID, CMPC_REFINE_ROUNDS, '
                   'CMPC_REFINE_CYCLE, CMPC_REFINE_MAX_ROUNDS);\n'
                   '  printf("%zu %zu\\n", sizeof(cmpc_gain_io), sizeof(cmpc_vjp_io));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    cc = shutil.which("cc") or shutil.which("gcc")
    cmd = [cc, str(src)] if cc else [hipcc(), "-x", "c", str(src)]
    subprocess.run(cmd + [f"-I{REPO / 'include'}", "-o", str(exe)], check=True, timeout=120)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True,
                                           timeout=60).stdout.split()]
    assert vals[0] == 6 == _lib.ABI_VERSION                      # no ABI bump
    assert vals[1] == ctypes.sizeof(_lib.CRefineIO)
    assert vals[2:-6] == [getattr(_lib.CRefineIO, n).offset for n in names]
    assert vals[-6:-2] == [-1, -2, -3, 16] == [_lib.REFINE_INVALID, _lib.REFINE_ROUNDS,
                                               _lib.REFINE_CYCLE, _lib.REFINE_MAX_ROUNDS]
    assert [refine_util.INVALID, refine_util.ROUNDS, refine_util.CYCLE] == [-1, -2, -3]
    assert vals[-2:] == [ctypes.sizeof(_lib.CGainIO), ctypes.sizeof(_lib.CVjpIO)]  # neighbours
    assert names == ["size", "Ad", "Bd", "gd", "x0", "xref", "contact", "mu", "fz_min", "Q", "R",
                     "w", "faces", "face_tol", "max_rounds", "prim_tol", "dual_tol", "info", "res",
                     "w64", "lam_out", "faces_out", "w_out", "status"]


def test_entry_is_declared_and_exported(lib):
    from cmpc import _lib, Plan
    from test_cabi import declared_symbols
    assert "cmpc_refine_run" in declared_symbols()
    assert "cmpc_refine_run" in _lib.EXPORTS and hasattr(lib, "cmpc_refine_run")
    assert callable(Plan.refine)


def _io(**fields):
    from cmpc import _lib
    io = _lib.CRefineIO()
    io.size = ctypes.sizeof(_lib.CRefineIO)
    for k in REQUIRED + ("w",):
        setattr(io, k, FAKE)
    io.max_rounds = 8
    for k, v in fields.items():
        setattr(io, k, v)
    return io


def _refused(lib, plan, io, B=1):
    from cmpc import _lib
    rc = lib.cmpc_refine_run(plan, B, None if io is None else ctypes.byref(io), None)
    msg = _lib.last_error(lib)
    assert rc == -22 and "cmpc_refine_run" in msg, (rc, msg)
    return msg


def test_argument_checks_come_before_the_plan(lib):
    from cmpc import _lib
    assert "null io" in _refused(lib, None, None)
    short = _io()
    short.size = _lib.CRefineIO.info.offset        # must reach past info
    assert "size" in _refused(lib, FAKE, short)
    assert "null plan" in _refused(lib, None, _io())
    for name in REQUIRED:
        assert "null array" in _refused(lib, FAKE, _io(**{name: None})), name
    assert "both null" in _refused(lib, FAKE, _io(w=None, faces=None))
    ends = _io(w=None, faces=None)                 # a struct that ends after info
    ends.size = _lib.CRefineIO.info.offset + ctypes.sizeof(ctypes.c_void_p)
    assert "both null" in _refused(lib, FAKE, ends)
    for rounds in (-1, 17, 1 << 20):
        assert "max_rounds" in _refused(lib, FAKE, _io(max_rounds=rounds)), rounds
    for tol in (-1e-9, float("nan"), float("inf"), -float("inf")):
        assert "face_tol" in _refused(lib, FAKE, _io(face_tol=tol)), tol
        assert "prim_tol" in _refused(lib, FAKE, _io(prim_tol=tol)), tol
        assert "dual_tol" in _refused(lib, FAKE, _io(dual_tol=tol, w=None, faces=FAKE)), tol
    assert "B must be" in _refused(lib, FAKE, _io(), B=0)
