"""GPU: ``Plan.solve`` reaches the kernels through one entry, ``cmpc_solve_io_run``; the
positional entries ``cmpc_solve`` / ``cmpc_solve_warm`` / ``cmpc_solve_ref`` stay in the ABI and
fill the same struct.  Every option of ``Plan.solve`` against a direct ctypes call of the entry
that used to serve it, into buffers of its own, bit for bit (``torch.equal``); then the identity
of ``out=`` tensors, the tuple lengths and the argument errors.

The batch is tests/golden/qp_terrain.npz: 34 instances, N = 16, with 7 / 18 / 4 / 3 / 2 instances
in the NC 96 / 128 / 144 / 160 / 192 bins, so with ``set_team(0)`` all three group kernels launch
and at the default it is one team launch.  Every comparison runs in both modes.
"""
import contextlib
import ctypes

import pytest
import torch

from parity_util import load_fixture

pytestmark = pytest.mark.gpu
KEYS = ("Ad", "Bd", "gd", "x0", "xref", "contact")
N = 16
TEAM_MODES = pytest.mark.parametrize("team", [-1, 0], ids=["team", "groups"])


@pytest.fixture(scope="module")
def data(plan):
    """The fixture on the device, its terrain set A, and a first solve's w / y / lam to warm
    start from (computed once, never written again)."""
    from cmpc import to_device_batch
    fx = load_fixture("qp_terrain.npz")
    d = to_device_batch({k: fx[k] for k in KEYS}, plan.device)
    d["mu"] = torch.as_tensor(fx["mu_A"], dtype=torch.float32).to(plan.device)
    d["fz_min"] = torch.as_tensor(fx["fz_min_A"], dtype=torch.float32).to(plan.device)
    args = tuple(d[k] for k in KEYS)
    d["w0"], _, _, d["y0"] = plan.solve(*args, y_out=True)
    d["lam0"] = plan.solve(*args, lam_out=True)[3]
    torch.cuda.synchronize(plan.device)
    return d


@contextlib.contextmanager
def team_mode(plan, team):
    """The session's plan with the team bound ``team``, the automatic bound restored after."""
    plan.set_team(team)
    try:
        B = 34
        assert (B <= plan.team_batch()) == (team == -1)
        assert all(plan.solve_kernels(B)) == (team == 0)
        yield
    finally:
        plan.set_team(-1)


def _args(d):
    return tuple(d[k] for k in KEYS)


def _buffers(plan, B, dual=0):
    """Fresh w, status, iters and, with ``dual`` columns, a dual buffer."""
    dev = plan.device
    bufs = [torch.empty((B, 24 * N), dtype=torch.float32, device=dev),
            torch.empty((B,), dtype=torch.int32, device=dev),
            torch.empty((B,), dtype=torch.int32, device=dev)]
    if dual:
        bufs.append(torch.empty((B, dual), dtype=torch.float32, device=dev))
    return bufs


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream(plan):
    return ctypes.c_void_p(torch.cuda.current_stream(plan.device).cuda_stream)


def _direct(plan, entry, d, init=(), dual=0):
    """``entry`` called through ctypes: cmpc_solve, or cmpc_solve_warm / cmpc_solve_ref with the
    two warm-start tensors ``init`` (None = NULL) and a dual output of ``dual`` columns."""
    B = d["Ad"].shape[0]
    bufs = _buffers(plan, B, dual)
    w, st, it = bufs[:3]
    if entry == "cmpc_solve":
        ptrs = [_ptr(t) for t in _args(d) + (w, st, it)]
    else:
        ptrs = [_ptr(t) for t in _args(d) + tuple(init) + (w, bufs[3], st, it)]
    with torch.cuda.device(plan.device):
        rc = getattr(plan.lib, entry)(plan._h, B, *ptrs, _stream(plan))
    assert rc == 0, plan.lib.cmpc_last_error().decode()
    return bufs


def _same(got, want):
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.data_ptr() != b.data_ptr()
        assert torch.equal(a, b), f"result {i} differs"


@TEAM_MODES
def test_plain_is_cmpc_solve(plan, data, team):
    with team_mode(plan, team):
        _same(plan.solve(*_args(data)), _direct(plan, "cmpc_solve", data))


@TEAM_MODES
@pytest.mark.parametrize("w_init,y_init", [(None, None), ("w0", "y0"), ("w0", None)],
                         ids=["cold", "warm", "primal"])
def test_y_out_is_cmpc_solve_warm(plan, data, team, w_init, y_init):
    init = tuple(None if k is None else data[k] for k in (w_init, y_init))
    with team_mode(plan, team):
        got = plan.solve(*_args(data), w_init=init[0], y_init=init[1], y_out=True)
        _same(got, _direct(plan, "cmpc_solve_warm", data, init, dual=12 * N))


@TEAM_MODES
@pytest.mark.parametrize("w_init,lam_init", [(None, None), ("w0", "lam0")], ids=["cold", "warm"])
def test_lam_out_is_cmpc_solve_ref(plan, data, team, w_init, lam_init):
    init = tuple(None if k is None else data[k] for k in (w_init, lam_init))
    with team_mode(plan, team):
        got = plan.solve(*_args(data), w_init=init[0], lam_init=init[1], lam_out=True)
        _same(got, _direct(plan, "cmpc_solve_ref", data, init, dual=52 * N))


@TEAM_MODES
def test_terrain_is_a_hand_filled_struct(plan, data, team):
    from cmpc import _lib
    B = data["Ad"].shape[0]
    w, st, it, y = _buffers(plan, B, dual=12 * N)
    io = _lib.CSolveIO()
    io.size = ctypes.sizeof(_lib.CSolveIO)
    for k in KEYS + ("mu", "fz_min"):
        setattr(io, k, data[k].data_ptr())
    io.w_out, io.status, io.iters, io.y_out = (t.data_ptr() for t in (w, st, it, y))
    with team_mode(plan, team):
        got = plan.solve(*_args(data), mu=data["mu"], fz_min=data["fz_min"], y_out=True)
        with torch.cuda.device(plan.device):
            rc = plan.lib.cmpc_solve_io_run(plan._h, B, ctypes.byref(io), _stream(plan))
        assert rc == 0, plan.lib.cmpc_last_error().decode()
        _same(got, (w, st, it, y))


def test_out_tensors_are_returned_and_tuple_lengths(plan, data):
    B = data["Ad"].shape[0]
    out = tuple(_buffers(plan, B))
    y, lam = (torch.empty((B, c * N), dtype=torch.float32, device=plan.device) for c in (12, 52))
    r = plan.solve(*_args(data), out=out)
    assert len(r) == 3 and all(a is b for a, b in zip(r, out))
    r = plan.solve(*_args(data), out=out, y_out=y)
    assert len(r) == 3 and all(a is b for a, b in zip(r, out))
    r = plan.solve(*_args(data), out=out, lam_out=lam)
    assert len(r) == 3 and all(a is b for a, b in zip(r, out))
    r = plan.solve(*_args(data), out=out, y_out=True)
    assert len(r) == 4 and all(a is b for a, b in zip(r, out)) and r[3].shape == (B, 12 * N)
    r = plan.solve(*_args(data), out=out, lam_out=True)
    assert len(r) == 4 and all(a is b for a, b in zip(r, out)) and r[3].shape == (B, 52 * N)
    torch.cuda.synchronize()


def test_duals_are_exclusive(plan, data):
    with pytest.raises(ValueError):
        plan.solve(*_args(data), lam_out=True, y_out=True)
    with pytest.raises(ValueError):
        plan.solve(*_args(data), lam_init=data["lam0"], y_init=data["y0"])
    with pytest.raises(ValueError):
        plan.solve(*_args(data), mu=data["mu"], lam_out=True, y_init=data["y0"])


def _bad(kind, shape, dtype, device):
    """A tensor that is right but for one property."""
    if kind == "dtype":
        wrong = torch.float64 if dtype == torch.float32 else torch.int64
        return torch.zeros(shape, dtype=wrong, device=device), TypeError
    if kind == "shape":
        return torch.zeros(shape[:-1] + (shape[-1] + 1,), dtype=dtype, device=device), ValueError
    if kind == "view":
        t = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=dtype, device=device)[..., ::2]
        assert tuple(t.shape) == tuple(shape) and not t.is_contiguous()
        return t, ValueError
    return torch.zeros(shape, dtype=dtype, device="cpu"), ValueError


@pytest.mark.parametrize("kind", ["dtype", "shape", "view", "cpu"])
@pytest.mark.parametrize("name,cols", [("w_init", 24 * N), ("y_init", 12 * N),
                                       ("lam_init", 52 * N), ("mu", 0), ("w", 24 * N),
                                       ("status", 0)])
def test_bad_tensor_raises(plan, data, name, cols, kind):
    """The exception types of the parent commit: TypeError for a dtype, ValueError for a shape, a
    non-contiguous view or a tensor that is not on the plan's device."""
    B = data["Ad"].shape[0]
    shape = (B, cols) if cols else (B,)
    dtype = torch.int32 if name == "status" else torch.float32
    t, exc = _bad(kind, shape, dtype, plan.device)
    if name in ("w", "status"):
        out = _buffers(plan, B)
        out[("w", "status").index(name)] = t
        kw = dict(out=tuple(out))
    else:
        kw = {name: t}
    with pytest.raises(exc):
        plan.solve(*_args(data), **kw)


def test_batch_past_max_batch(data):
    from cmpc import CmpcError, Plan, SolverParams
    small = Plan(SolverParams(max_batch=8), device=data["Ad"].device)
    try:
        with pytest.raises(CmpcError, match="max_batch"):
            small.solve(*_args(data))
    finally:
        small.close()
