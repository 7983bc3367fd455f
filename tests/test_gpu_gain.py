"""GPU: feedback gain, value-function derivatives and the optimum on the held faces of a batch
(cmpc_gain_run / Plan.gain, include/cmpc.h) against the two float64 NumPy references of
tests/gain_util.py on the same fp32-rounded arrays.

Bar (gain_util): |dev - ref| <= 1e-8 x scale per output.  Every instance is held to it against
reference (a), the dense KKT solve, and against reference (b), the NumPy Riccati recursion, which
test_gain.py ties to (a) within 1e-9 x scale."""
import ctypes

import numpy as np
import pytest
import torch

from parity_util import load_fixture
import gain_util
import kkt_util

pytestmark = pytest.mark.gpu
IN = ("Ad", "Bd", "gd", "x0", "xref", "contact")
ALL = ("K", "Vx", "Vxx", "u_star", "faces")
_cache = {}


def _dev(plan, a):
    return torch.as_tensor(np.ascontiguousarray(a)).contiguous().to(plan.device)


def _gain(plan, case, idx=None, want=ALL, use_w=True, faces=None, **over):
    """Plan.gain on (the instances idx of) a case -> dict of numpy arrays."""
    sel = (lambda a: a) if idx is None else (lambda a: a[idx])
    kw = {k: _dev(plan, sel(case[k])) for k in ("mu", "fz_min", "Q", "R") if k in case}
    kw.update({k: (_dev(plan, v) if isinstance(v, np.ndarray) else v) for k, v in over.items()})
    out = plan.gain(*[_dev(plan, sel(case[k])) for k in IN],
                    w=_dev(plan, sel(case["w"])) if use_w else None,
                    faces=None if faces is None else _dev(plan, sel(faces)), want=want, **kw)
    torch.cuda.synchronize(plan.device)
    B, N = len(sel(case["Ad"])), case["Bd"].shape[1]
    shapes = dict(K=(B, 12, 12), Vx=(B, 12), Vxx=(B, 12, 12), u_star=(B, 12 * N), faces=(B, N, 4))
    assert set(out) == set(want) | {"K"}
    for n, t in out.items():
        assert tuple(t.shape) == shapes[n] and t.dtype == (torch.uint8 if n == "faces" else
                                                          torch.float64), n
    return {n: t.cpu().numpy() for n, t in out.items()}


def _check(dev, case, faces, params, rows, dense_rows, what):
    """Instances `rows` of dev against reference (b), `dense_rows` also against (a); prints the
    worst ratio per output and reference before asserting.  -> the worst ratios against (a)."""
    worst = {"a": {n: 0.0 for n in gain_util.OUTPUTS}, "b": {n: 0.0 for n in gain_util.OUTPUTS}}
    for i in rows:
        iv = kkt_util.instance_values(case, i, params)
        args, kw = gain_util.instance_args(case, i, iv)
        mine = {n: dev[n][i] for n in gain_util.OUTPUTS if n in dev}
        assert all(np.all(np.isfinite(v)) for v in mine.values()), (what, i)
        ric = gain_util.ref_riccati(*args, faces[i], **kw)
        vals, S = gain_util.ref_dense(*args, faces[i], **kw) if i in dense_rows else (None, None)
        if S is None:       # the scales of (a) from (b)'s values (they agree to 1e-9 x scale)
            S = dict(K=max(1.0, float(np.abs(ric["K"]).max())),
                     u_star=gain_util.force_scale(ric["u_star"]))
            mine = {n: mine[n] for n in S if n in mine}
        else:
            for n, r in gain_util.worst_ratio(mine, vals, S).items():
                worst["a"][n] = max(worst["a"][n], r)
        for n, r in gain_util.worst_ratio(mine, ric, S).items():
            worst["b"][n] = max(worst["b"][n], r)
    print(what, "worst |dev - ref| / (1e-8 scale): dense KKT (a)", worst["a"], "riccati (b)",
          worst["b"])
    assert max(worst["a"].values()) <= 1.0 and max(worst["b"].values()) <= 1.0, (what, worst)
    return worst["a"]


def _fixture(plan, name, tag):
    key = (name, tag)
    if key not in _cache:
        case = kkt_util.fixture_case(load_fixture(name), tag, plan.params)
        faces = np.stack([gain_util.classify(case["contact"][i], case["w"][i], **{
            k: kkt_util.instance_values(case, i, plan.params)[k] for k in ("mu", "fz_min")})
            for i in range(len(case["w"]))])
        _cache[key] = (case, faces)
    return _cache[key]


@pytest.mark.parametrize("name,tag", kkt_util.FIXTURES)
def test_fixtures_faces_from_w(plan, name, tag):
    """The five fixture sets with their per-instance mu / fz_min / Q / R, faces read off w
    (test_kkt.py guards that no face test of these sets sits on its threshold)."""
    case, faces = _fixture(plan, name, tag)
    dev = _gain(plan, case)
    assert np.array_equal(dev["faces"], faces)
    B = len(faces)
    _check(dev, case, faces, plan.params, range(B), set(range(B)), f"{name}{tag}")
    # K alone (one LDS slot instead of N) and the faces given back are bitwise the same
    assert np.array_equal(_gain(plan, case, want=("K",))["K"], dev["K"])
    again = _gain(plan, case, use_w=False, faces=faces)
    assert all(np.array_equal(again[n], dev[n]) for n in ALL)
    assert np.array_equal(_gain(plan, case, want=("K",), face_tol=0.0)["K"], dev["K"])
    # another tolerance is honoured: at 1e3 every stance leg holds fz_min and the + faces
    loose = _gain(plan, case, idx=np.arange(2), want=("K", "faces"), face_tol=1e3)
    stance = case["contact"][:2].transpose(0, 2, 1) != 0
    assert np.all(loose["faces"][stance] == 11) and np.all(loose["faces"][~stance] == 0)
    assert np.all(loose["K"] == 0.0)


def random_case(N, B=67, seed=23):
    """Arbitrary problems and face sets (nothing is a solution), fp32, with per-instance
    mu / fz_min / Q / R.  Special instances: 0 has every leg in swing on the even steps and leg 0 fully
    pinned on the odd ones; 1 has every stance leg fully pinned (no free parameter at all); 2 has
    fz_min = 0 and both-sign masks; 5 an invalid mu, 6 an invalid R row; every seventh instance
    from 3 on carries one inconsistent mask (both signs of an axis with bit 0, fz_min != 0).
    No other stance leg has an inconsistent mask."""
    rng = np.random.default_rng(seed + N)
    c = dict(Ad=np.eye(12) + 0.05 * rng.standard_normal((B, 12, 12)),
             Bd=0.1 * rng.standard_normal((B, N, 12, 12)), gd=0.1 * rng.standard_normal((B, 12)),
             x0=rng.standard_normal((B, 12)), xref=rng.standard_normal((B, N, 12)),
             mu=rng.uniform(0.2, 1.0, B), fz_min=rng.uniform(1.0, 20.0, B),
             Q=rng.uniform(0.0, 50.0, (B, 12)), R=rng.uniform(1e-4, 1e-2, (B, 12)))
    c["fz_min"][2::9] = 0.0
    c = {k: kkt_util.f32(v) for k, v in c.items()}
    ct = (rng.random((B, 4, N)) < 0.7).astype(np.uint8)
    ct[0, 0, :] = 1
    ct[0, :, ::2] = 0
    ct[1] = 1
    c["contact"] = ct
    faces = rng.integers(0, 32, (B, N, 4)).astype(np.uint8)
    faces[rng.random(faces.shape) < 0.35] = 0
    faces[0, :, 0] = 1 | 2 | 16
    faces[1] = 1 | 4 | 8
    faces[2] = rng.choice([6, 24, 30, 7, 25, 31, 6 | 8, 24 | 2], (N, 4))
    both = ((faces & 6) == 6) | ((faces & 24) == 24)
    bad = both & ((faces & 1) != 0) & (c["fz_min"] != 0)[:, None, None]
    faces[bad] &= 0xFE
    faces |= rng.integers(0, 8, faces.shape).astype(np.uint8) << 5      # bits 5..7 are ignored
    nan_rows = [5, 6] + list(range(3, B, 7))
    for b in range(3, B, 7):
        if c["fz_min"][b] == 0:
            c["fz_min"][b] = np.float32(3.0)
        k = int(rng.integers(N))
        ct[b, 1, k] = 1
        faces[b, k, 1] = 1 | 2 | 4
    c["mu"][5] = np.float32(-0.5)
    c["R"][6, 7] = np.float32(0.0)
    return c, faces, sorted(set(r for r in nan_rows if r < B))


def _expected_faces(c, faces, nan_rows):
    want = faces & 31
    want[c["contact"].transpose(0, 2, 1) == 0] = 0
    want[nan_rows] = 0xFF
    return want


@pytest.mark.parametrize("N", [1, 5, 16])
def test_arbitrary_face_sets_given(N):
    from cmpc import Plan, SolverParams, _lib
    plan = Plan(SolverParams(N=N, max_batch=8))     # (max_batch does not limit B)
    c, faces, nan_rows = random_case(N)
    B = len(faces)
    good = [i for i in range(B) if i not in nan_rows]
    for i in range(B):      # the generator's promise: exactly nan_rows 3, 10, .. are inconsistent
        ok = gain_util.consistent(faces[i], c["contact"][i], float(c["mu"][i]), float(c["fz_min"][i]))
        assert ok == (i not in nan_rows or i in (5, 6)), i
    dev = _gain(plan, c, use_w=False, faces=faces)
    assert np.array_equal(dev["faces"], _expected_faces(c, faces, nan_rows))
    for n in gain_util.OUTPUTS:
        assert np.all(np.isnan(dev[n][nan_rows])), n
        assert np.all(np.isfinite(dev[n][good])), n
    _check(dev, c, faces, plan.params, good, set(good), f"N={N} B={B}")
    assert np.all(dev["K"][1] == 0.0)                       # no free parameter: a zero gain
    u1 = dev["u_star"][1].reshape(N, 4, 3)                  # and every force on its pinned point
    fz, mu = float(c["fz_min"][1]), float(c["mu"][1])
    assert np.allclose(u1, [-mu * fz, mu * fz, fz], rtol=1e-15, atol=0)
    swing = c["contact"].transpose(0, 2, 1)[good] == 0
    assert np.all(dev["u_star"][good].reshape(len(good), N, 4, 3)[swing] == 0.0)
    # smaller batches of the same instances: bitwise the same rows (independent of B and place)
    for idx in ([2, 5, 6], [0], [5], [3]):
        idx = np.array(idx)
        sub = _gain(plan, c, idx=idx, use_w=False, faces=faces)
        for n in ALL:
            assert np.array_equal(sub[n], dev[n][idx], equal_nan=True), (n, idx)
    # a struct that stops after K: K is computed, nothing past it is written
    t = {k: _dev(plan, c[k]) for k in IN + ("mu", "fz_min", "Q", "R")}
    t["faces"] = _dev(plan, faces)
    K = torch.zeros((B, 12, 12), dtype=torch.float64, device=plan.device)
    guard = torch.full((B, 12 * N), 7.0, dtype=torch.float64, device=plan.device)
    io = _lib.CGainIO()
    for k, v in t.items():
        setattr(io, k, v.data_ptr())
    io.K = K.data_ptr()
    io.Vx = io.Vxx = io.u_star = io.faces_out = guard.data_ptr()
    io.size = _lib.CGainIO.K.offset + ctypes.sizeof(ctypes.c_void_p)
    with torch.cuda.device(plan.device):
        rc = plan.lib.cmpc_gain_run(plan._h, ctypes.c_int64(B), ctypes.byref(io), ctypes.c_void_p(
            torch.cuda.current_stream(plan.device).cuda_stream))
    torch.cuda.synchronize(plan.device)
    assert rc == 0, _lib.last_error(plan.lib)
    assert np.array_equal(K.cpu().numpy(), dev["K"], equal_nan=True)
    assert torch.all(guard == 7.0)
    plan.close()


def test_the_law_is_affine_in_x0(plan):
    """With the faces fixed, u_star(x0 + d) - u_star(x0) = K d on the first step, for
    displacements that are not small.  Tolerance: each of the two u_star is within the bar of
    its exact value (1e-8 x max|u|) and K within 1e-8 x max(1, max|K|) per entry, so the
    difference is held to 1e-8 x (2 max|u| + max(1, max|K|) x |d|_1)."""
    case, faces = _fixture(plan, "qp_cfg2.npz", "")
    idx = np.arange(0, 64, 4)
    base = _gain(plan, case, idx=idx, use_w=False, faces=faces, want=("K", "u_star"))
    rng = np.random.default_rng(3)
    x0 = case["x0"][idx]
    worst = 0.0
    for size in (0.05, 0.5, 3.0):
        moved = dict(case)
        moved["x0"] = case["x0"].copy()
        moved["x0"][idx] = kkt_util.f32(x0 + size * rng.uniform(-1.0, 1.0, x0.shape))
        d = moved["x0"][idx].astype(np.float64) - x0.astype(np.float64)
        assert np.abs(d).max() > 0.5 * size
        got = _gain(plan, moved, idx=idx, use_w=False, faces=faces, want=("K", "u_star"))
        assert np.array_equal(got["K"], base["K"])             # K does not depend on x0
        du = got["u_star"][:, :12] - base["u_star"][:, :12]
        Kd = np.einsum("bij,bj->bi", base["K"], d)
        assert np.abs(Kd).max() > 1.0
        umax = np.maximum(np.abs(got["u_star"]).max(axis=1), np.abs(base["u_star"]).max(axis=1))
        Kmax = np.maximum(1.0, np.abs(base["K"]).max(axis=(1, 2)))
        tol = gain_util.TOL_REL * (2.0 * umax + Kmax * np.abs(d).sum(axis=1))
        ratio = np.abs(du - Kd).max(axis=1) / tol
        print("size", size, "max |K d|", np.abs(Kd).max(), "worst |du - K d| / tol", ratio.max())
        worst = max(worst, ratio.max())
    assert worst <= 1.0


def test_repeatable_and_position_independent(plan):
    case, faces = _fixture(plan, "qp_terrain.npz", "_A")
    a, b = _gain(plan, case), _gain(plan, case)
    assert all(np.array_equal(a[n], b[n]) for n in ALL)
    rev = {k: (v[::-1].copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    r = _gain(plan, rev)
    assert all(np.array_equal(r[n][::-1], a[n]) for n in ALL)
    perm = np.random.default_rng(1).permutation(len(faces))
    p = _gain(plan, case, idx=perm)
    assert all(np.array_equal(p[n], a[n][perm]) for n in ALL)
    # and a tile of the batch past one grid-stride pass of the kernel (8192 blocks)
    reps = 8192 // len(faces) + 2
    big = _gain(plan, {k: np.tile(v, (reps,) + (1,) * (v.ndim - 1)) for k, v in case.items()
                       if isinstance(v, np.ndarray)})
    assert all(np.array_equal(big[n], np.tile(a[n], (reps,) + (1,) * (a[n].ndim - 1))) for n in ALL)


def test_end_to_end_solve_then_gain(plan):
    """64 instances of config 2 solved, then the gain on the device's own w_out."""
    from cmpc import synth, to_device_batch
    from oracle import active_set
    batch = synth.make_config(2, B=64)
    d = to_device_batch(batch, plan.device)
    args = [d[k] for k in IN]
    w, st, it = plan.solve(*args)
    out = plan.gain(*args, w=w, want=ALL)
    torch.cuda.synchronize(plan.device)
    st = st.cpu().numpy()
    assert np.all((st == 1) | (st == 2))
    case = {k: d[k].cpu().numpy() for k in IN}
    case["w"] = w.cpu().numpy()
    dev = {n: t.cpu().numpy() for n, t in out.items()}
    pc = kkt_util.plan_constants(plan.params)
    B, N = 64, plan.params.N
    # faces_out is the NumPy classification wherever the tested value is clear of its threshold
    mine = np.stack([gain_util.classify(case["contact"][i], case["w"][i], pc["mu"], pc["fz_min"])
                     for i in range(B)])
    gap = np.stack([gain_util.threshold_gap(case["contact"][i], case["w"][i], pc["mu"],
                                            pc["fz_min"]) for i in range(B)])
    clear = gap > 1e-9
    print("legs within 1e-9 of a face threshold:", int((~clear & np.isfinite(gap)).sum()))
    assert np.array_equal(dev["faces"][clear], mine[clear])
    # the device against the references built on the device's own faces_out
    _check(dev, case, dev["faces"], plan.params, range(B), set(range(B)), "solve output")
    # printed, not asserted: the float64 optimum on the recovered faces against w_out and
    # against the certified optimum of the whole QP
    U = case["w"][:, 12 * N:].astype(np.float64)
    print("max |u_star - w_out forces| / max|u| over status 1:",
          float(np.max(np.abs(dev["u_star"] - U)[st == 1] /
                       np.abs(U).max(axis=1, keepdims=True)[st == 1])))
    same, dist = 0, 0.0
    sample = range(0, B, 8)
    for i in sample:
        r = active_set.certify_batch_item(batch, i, case["w"][i].astype(np.float64))
        wo = np.asarray(r["w"], np.float64)
        same += int(np.array_equal(gain_util.classify(case["contact"][i], wo, pc["mu"], pc["fz_min"]),
                                   dev["faces"][i]))
        dist = max(dist, float(np.abs(dev["u_star"][i] - wo[12 * N:]).max() / np.abs(wo[12 * N:]).max()))
    print("certified optimum (oracle.active_set) on", len(sample), "instances: recovered faces equal "
          "its active set on", same, "; max |u_star - u_opt| / max|u|:", dist)


def test_closed_loop_gain_in_a_captured_tick(plan):
    from cmpc.closed_loop import ClosedLoop
    B = 8
    loop = ClosedLoop(B, plan=plan, seed=4, gain=True)
    cmd = np.zeros((B, 4), np.float32)
    cmd[:, 0], cmd[:, 2], cmd[:, 3] = 0.4, 0.27, 1.0
    loop.set_command(cmd)
    assert tuple(loop.K0.shape) == (B, 12, 12) and loop.K0.dtype == torch.float64
    assert loop.report is False and not hasattr(loop, "kkt")

    def check():
        torch.cuda.synchronize(loop.dev)
        want = plan.gain(loop.Ad, loop.Bd, loop.gd, loop.x_solve, loop.xref, loop.ct, w=loop.w)["K"]
        torch.cuda.synchronize(loop.dev)
        assert torch.equal(loop.K0, want)
        assert not torch.equal(loop.x_solve, loop.x)             # the plant has moved x on
        k = loop.K0.cpu().numpy()
        assert np.all(np.isfinite(k)) and np.abs(k).max() > 1.0
        return k

    loop.tick()
    ks = [check()]
    loop.capture()
    for _ in range(2):
        loop.tick()
        ks.append(check())
    assert not np.array_equal(ks[-1], ks[-2]) and not np.array_equal(ks[1], ks[0])
    plain = ClosedLoop(B, plan=plan, seed=4)
    assert plain.gain is False and not hasattr(plain, "K0") and not hasattr(plain, "x_solve")
