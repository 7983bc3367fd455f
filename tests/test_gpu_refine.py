"""GPU: the certified float64 refinement of a solved batch (cmpc_refine_run / Plan.refine,
include/cmpc.h) against the NumPy model of tests/refine_util.py on the same fp32-rounded arrays,
and against oracle.active_set.

Bars (refine_util): forces within 1e-8 x max|u| of the model's, states within 1e-8 x
max(1, max|x|), multipliers within 1e-8 x the largest sum of absolute terms of g; info and the
masks exactly wherever the model's decisions are clear of their thresholds by a factor of 2.  A
certified row against the oracle: the model's 1e-10 plus the device's 1e-8, x max|u|."""
import numpy as np
import pytest
import torch

from parity_util import load_fixture
import gain_util
import kkt_util
import refine_util

pytestmark = pytest.mark.gpu
IN = ("Ad", "Bd", "gd", "x0", "xref", "contact")
ALL = ("info", "res", "w64", "lam", "faces")
TOL = gain_util.TOL_REL
_cache = {}


def _dev(plan, a):
    return torch.as_tensor(np.ascontiguousarray(a)).contiguous().to(plan.device)


def _refine(plan, case, idx=None, want=ALL, use_w=True, faces=None, w_out=None, status=None, **over):
    """Plan.refine on (the instances idx of) a case -> dict of numpy arrays; w_out / status
    (numpy, copied to the device) come back under those names; w_out="alias" passes w itself."""
    sel = (lambda a: a) if idx is None else (lambda a: a[idx])
    kw = {k: _dev(plan, sel(case[k])) for k in ("mu", "fz_min", "Q", "R") if k in case}
    kw.update(over)
    w = _dev(plan, sel(case["w"])) if use_w else None
    wo = w if isinstance(w_out, str) else (None if w_out is None else _dev(plan, w_out))
    st = None if status is None else _dev(plan, status)
    out = plan.refine(*[_dev(plan, sel(case[k])) for k in IN], w=w,
                      faces=None if faces is None else _dev(plan, sel(faces)), w_out=wo,
                      status=st, want=want, **kw)
    torch.cuda.synchronize(plan.device)
    B, N = len(sel(case["Ad"])), case["Bd"].shape[1]
    shapes = dict(info=(B,), res=(B, 3), w64=(B, 24 * N), lam=(B, 52 * N), faces=(B, N, 4))
    dtypes = dict(info=torch.int32, faces=torch.uint8)
    assert set(out) == set(want) | {"info"}
    for n, t in out.items():
        assert tuple(t.shape) == shapes[n] and t.dtype == dtypes.get(n, torch.float64), n
    res = {n: t.cpu().numpy() for n, t in out.items()}
    if wo is not None:
        res["w_out"] = wo.cpu().numpy()
    if st is not None:
        res["status"] = st.cpu().numpy()
    return res


def _against_model(dev, ref, i, N, what):
    """Row i of the device's outputs against the model's dict ref, within the bars."""
    us = gain_util.force_scale(ref["u"])
    xs = max(1.0, float(np.abs(ref["x"]).max()))
    w64 = dev["w64"][i]
    r = dict(u=np.abs(w64[12 * N:] - ref["u"]).max() / (TOL * us),
             x=np.abs(w64[:12 * N] - ref["x"].reshape(-1)).max() / (TOL * xs),
             lam=np.abs(dev["lam"][i] - ref["lam"]).max() / (TOL * ref["lam_scale"]))
    # res[0] = violation / us, res[1] = multiplier / gs: the bars of u and lam divided by us, gs
    usc = max(1.0, float(np.abs(ref["u"]).max()))
    r["res0"] = abs(dev["res"][i, 0] - ref["res"][0]) / (TOL * 2.0 * us / usc)
    r["res1"] = abs(dev["res"][i, 1] - ref["res"][1]) / (TOL * ref["lam_scale"] * ref["res_gs_inv"])
    if np.isnan(ref["res"][2]):
        assert np.isnan(dev["res"][i, 2]), (what, i)
    else:
        r["res2"] = abs(dev["res"][i, 2] - ref["res"][2]) / (TOL * us)
    assert max(r.values()) <= 1.0, (what, i, r)
    return r


def _model_rows(case, params, rows, faces=None, **kw):
    out = {}
    for i in rows:
        o = refine_util.model_case(case, i, params, faces=None if faces is None else faces[i], **kw)
        iv = kkt_util.instance_values(case, i, params)
        if o["info"] != refine_util.INVALID:
            o["res_gs_inv"] = 1.0 / (max(1.0, np.abs(o["u"]).max()) * 2.0 * iv["R"].min())
        out[i] = o
    return out


def _compare(dev, model, N, what, exact_rows=None):
    """Every modelled row: info and masks exactly (on exact_rows, default all), values in the bars."""
    worst = {}
    for i, ref in model.items():
        if exact_rows is None or i in exact_rows:
            assert dev["info"][i] == ref["info"], (what, i, dev["info"][i], ref["info"])
            assert np.array_equal(dev["faces"][i], ref["faces"]), (what, i)
        elif not (dev["info"][i] == ref["info"] and np.array_equal(dev["faces"][i], ref["faces"])):
            continue                    # an unclear decision went the other way: another point
        if ref["info"] == refine_util.INVALID:
            for n in ("res", "w64", "lam"):
                assert np.all(np.isnan(dev[n][i])), (what, i, n)
            continue
        for k, v in _against_model(dev, ref, i, N, what).items():
            worst[k] = max(worst.get(k, 0.0), float(v))
    print(what, "worst |dev - model| / bar:", worst)


def _oracle_u(case, i, params, N):
    r = refine_util.oracle_optimum(case, i, params, case["w"][i])
    assert not r["fallback"]
    return r, r["w"][12 * N:]


def _fixture(plan, name, tag):
    key = (name, tag)
    if key not in _cache:
        case = kkt_util.fixture_case(load_fixture(name), tag, plan.params)
        _cache[key] = (case, _model_rows(case, plan.params, range(len(case["w"]))))
    return _cache[key]


@pytest.mark.parametrize("name,tag", kkt_util.FIXTURES)
def test_fixtures_faces_from_w(plan, name, tag):
    """1. The five fixture sets with their per-instance mu / fz_min / Q / R, faces read off w
    (test_kkt.py guards that no face test of these sets sits on its threshold)."""
    from oracle import active_set, mpc_qp
    case, model = _fixture(plan, name, tag)
    B, N = len(case["w"]), case["Bd"].shape[1]
    clear = {i for i, o in model.items() if o["margin"] >= refine_util.CLEAR}
    assert B - len(clear) <= 0.05 * B
    guard = np.full((B, 24 * N), 7.0, np.float32)
    dev = _refine(plan, case, w_out=guard, status=np.full(B, 5, np.int32))
    _compare(dev, model, N, f"{name}{tag}", exact_rows=clear)
    info = dev["info"]
    print(name, tag, "info", dict(zip(*np.unique(info, return_counts=True))))
    cert = info >= 0
    assert all(o["info"] >= 0 for o in model.values()) and np.all(cert)   # every instance
    assert np.array_equal(dev["w_out"][cert], dev["w64"][cert].astype(np.float32))
    assert np.all(dev["w_out"][~cert] == 7.0)
    assert np.array_equal(dev["status"], np.where(cert, 1, 5))
    for i in np.flatnonzero(cert)[::8]:
        iv = kkt_util.instance_values(case, i, plan.params)
        f64 = [np.asarray(case[k][i], np.float64) for k in ("Ad", "Bd", "gd", "x0", "xref")]
        qp = mpc_qp.build_qp(f64[0], f64[1], f64[2], f64[3], f64[4].T, case["contact"][i], **iv)
        kkt = mpc_qp.kkt_residuals(qp, dev["w64"][i], dev["lam"][i, :24 * N], dev["lam"][i, 24 * N:])
        assert max(kkt.values()) <= active_set.CERT_TOL, (i, kkt)
    # info alone, and the masks given back with w: bitwise the same
    assert np.array_equal(_refine(plan, case, want=("info",))["info"], info)
    again = _refine(plan, case, faces=dev["faces"])
    assert np.all(again["info"][cert] == 0)
    assert all(np.array_equal(again[n][cert], dev[n][cert]) for n in ("res", "w64", "lam", "faces"))
    only = _refine(plan, case, use_w=False, faces=dev["faces"])
    assert np.all(np.isnan(only["res"][:, 2]))
    assert np.array_equal(only["w64"][cert], dev["w64"][cert])
    assert np.array_equal(only["res"][cert, :2], dev["res"][cert, :2])


@pytest.mark.parametrize("name", ("qp_cfg2.npz", "qp_nc192.npz"))
@pytest.mark.parametrize("max_rounds", (0, 2, 8))
def test_wrong_face_seeds_given(plan, name, max_rounds):
    """2., 3. One wrong face per instance given as `faces` (a dropped one in the first half of
    the set, an added one in the second).  info and faces_out equal the model's wherever its
    decisions are clear by a factor of 2 (at most 5 % are not); certified rows equal the oracle,
    get status 1 and the rounded point; every other row of w_out (aliased to w, and separate) and
    of status is bit for bit what went in."""
    params = plan.params
    case = kkt_util.fixture_case(load_fixture(name), "", params)
    B, N = len(case["w"]), case["Bd"].shape[1]
    key = (name, "seeds")
    if key not in _cache:
        f0 = np.stack([gain_util.classify(case["contact"][i], case["w"][i], **{
            k: kkt_util.plan_constants(params)[k] for k in ("mu", "fz_min")}) for i in range(B)])
        seeds = refine_util.wrong_face_seeds(f0, case["contact"], "drop")
        seeds[B // 2:] = refine_util.wrong_face_seeds(f0, case["contact"], "add")[B // 2:]
        _cache[key] = seeds
    seeds = _cache[key]
    model = _model_rows(case, params, range(B), faces=seeds, max_rounds=max_rounds)
    clear = {i for i, o in model.items() if o["margin"] >= refine_util.CLEAR}
    print(name, max_rounds, "unclear instances:", B - len(clear))
    assert B - len(clear) <= 0.05 * B
    st_in = np.arange(B, dtype=np.int32) + 100
    dev = _refine(plan, case, faces=seeds, w_out="alias", status=st_in, max_rounds=max_rounds)
    sep = _refine(plan, case, faces=seeds, w_out=np.full((B, 24 * N), 7.0, np.float32),
                  max_rounds=max_rounds)
    _compare(dev, model, N, f"{name} rounds {max_rounds}", exact_rows=clear)
    info = dev["info"]
    print("info", dict(zip(*np.unique(info, return_counts=True))))
    assert set(info[info < 0]) <= {refine_util.ROUNDS}.union({refine_util.CYCLE})
    assert np.all(info <= max_rounds)
    cert = info >= 0
    assert np.array_equal(dev["status"], np.where(cert, 1, st_in))
    assert np.array_equal(dev["w_out"][cert], dev["w64"][cert].astype(np.float32))
    assert np.array_equal(dev["w_out"][~cert].view(np.uint32), case["w"][~cert].view(np.uint32))
    assert np.array_equal(sep["w_out"][cert], dev["w_out"][cert])
    assert np.all(sep["w_out"][~cert] == 7.0)
    assert all(np.array_equal(sep[n], dev[n], equal_nan=True) for n in ALL)
    for i in np.flatnonzero(cert)[::4]:
        _, uo = _oracle_u(case, i, params, N)
        err = np.abs(dev["w64"][i, 12 * N:] - uo).max() / np.abs(uo).max()
        assert err <= TOL + refine_util.ORACLE_REL, (i, err)
        assert abs(dev["res"][i, 2] - np.abs(uo - case["w"][i, 12 * N:]).max() /
                   max(1.0, np.abs(case["w"][i, 12 * N:]).max())) <= 2 * TOL * np.abs(uo).max()


def _random_case(N):
    """test_gpu_gain.random_case's problems with single-sign masks (what the refinement takes)
    on every instance but the invalid ones: 3, 10, .. keep one both-signs mask (inconsistent), 4
    gets a consistent one (fz_min = 0 would allow it in cmpc_gain_run), 5 an invalid mu, 6 an
    invalid R row."""
    from test_gpu_gain import random_case
    c, faces, nan_rows = random_case(N)
    keep = faces.copy()
    f = faces & 31
    f = np.where((f & 6) == 6, f & ~np.uint8(4), f)
    f = np.where((f & 24) == 24, f & ~np.uint8(16), f).astype(np.uint8)
    f |= faces & 0xE0
    for b in nan_rows:
        f[b] = keep[b]
    c["fz_min"][7] = np.float32(np.nan)
    c["Q"][8, 3] = np.float32(-1.0)
    ct = c["contact"]
    ct[4, 2, 0] = 1
    f[4, 0, 2] = 8 | 16
    return c, f, sorted(set(nan_rows) | {4, 7, 8})


@pytest.mark.parametrize("N", [1, 5, 16])
def test_arbitrary_single_sign_masks_and_invalid_entries(N):
    """4., 5. Arbitrary consistent single-sign masks on random problems (nothing is a solution),
    max_rounds = 4, against the model; invalid entries (mu <= 0, NaN fz_min, a negative Q, R = 0,
    an inconsistent mask, a both-signs mask) get info -1, NaN and 0xFF and leave their
    neighbours as they are."""
    from cmpc import Plan, SolverParams
    plan = Plan(SolverParams(N=N, max_batch=8))     # (max_batch does not limit B)
    c, faces, bad = _random_case(N)
    B = len(faces)
    c["w"] = kkt_util.f32(np.random.default_rng(N).standard_normal((B, 24 * N)))
    good = [i for i in range(B) if i not in bad]
    model = _model_rows(c, plan.params, range(B), faces=faces, max_rounds=4)
    assert all(model[i]["info"] == refine_util.INVALID for i in bad)
    assert all(model[i]["info"] != refine_util.INVALID for i in good)
    clear = {i for i, o in model.items() if o["margin"] >= refine_util.CLEAR}
    print("N", N, "unclear instances:", B - len(clear), "model info",
          dict(zip(*np.unique([o["info"] for o in model.values()], return_counts=True))))
    assert B - len(clear) <= 0.05 * B
    st_in = np.arange(B, dtype=np.int32) + 100
    dev = _refine(plan, c, faces=faces, w_out="alias", status=st_in, max_rounds=4)
    _compare(dev, model, N, f"N={N}", exact_rows=clear)
    assert np.all(dev["info"][bad] == -1) and np.all(dev["faces"][bad] == 0xFF)
    cert = dev["info"] >= 0
    assert np.array_equal(dev["status"], np.where(cert, 1, st_in))
    assert np.array_equal(dev["w_out"][~cert].view(np.uint32), c["w"][~cert].view(np.uint32))
    assert np.array_equal(dev["w_out"][cert], dev["w64"][cert].astype(np.float32))
    swing = c["contact"].transpose(0, 2, 1)[good] == 0
    assert np.all(dev["faces"][good][swing] == 0)
    # the neighbours of the invalid rows: bitwise the rows of a batch without them
    sub = _refine(plan, c, idx=np.array(good), faces=faces, max_rounds=4)
    for n in ALL:
        assert np.array_equal(sub[n], dev[n][good], equal_nan=True), n
    plan.close()


@pytest.mark.parametrize("N", [1, 5, 16])
def test_check_only_point_is_gains_u_star_bitwise(N):
    """With the masks given and max_rounds = 0 the refinement's point is Plan.gain's u_star: both
    run csrc/cmpc_lq.h's recursion and the same rollout arithmetic, so the forces agree byte for
    byte on every row both evaluate, and the rows they decline coincide -- but for row 4, whose
    both-signs mask without the fz face is consistent: gain evaluates it at fz = 0, the
    refinement declines every apex."""
    from cmpc import Plan, SolverParams
    plan = Plan(SolverParams(N=N, max_batch=8))
    c, faces, bad = _random_case(N)
    idx = np.arange(64)
    bad = [b for b in bad if b < 64]
    r = _refine(plan, c, idx=idx, want=("w64",), use_w=False, faces=faces, max_rounds=0)["w64"][:, 12 * N:]
    kw = {k: _dev(plan, c[k][idx]) for k in ("mu", "fz_min", "Q", "R")}
    g = plan.gain(*[_dev(plan, c[k][idx]) for k in IN], faces=_dev(plan, faces[idx]),
                  want=("u_star",), **kw)["u_star"].cpu().numpy()
    fin_r, fin_g = np.isfinite(r).all(1), np.isfinite(g).all(1)
    assert np.array_equal(np.flatnonzero(np.isnan(r).all(1)), bad) and np.all(fin_r[~np.isnan(r).all(1)])
    assert np.array_equal(np.flatnonzero(np.isnan(g).all(1)), [b for b in bad if b != 4])
    assert np.all(fin_g[~np.isnan(g).all(1)])
    both = fin_r & fin_g
    assert both.sum() == 64 - len(bad)
    assert np.array_equal(r[both].view(np.uint64), g[both].view(np.uint64))
    plan.close()


def test_argument_checks(plan):
    """5. The CMPC_E_INVALID cases reach the caller as CmpcError (ValueError where the binding
    refuses first)."""
    from cmpc import CmpcError
    case, _ = _fixture(plan, "qp_cfg2.npz", "")
    args = [_dev(plan, case[k][:2]) for k in IN]
    w = _dev(plan, case["w"][:2])
    with pytest.raises(ValueError):
        plan.refine(*args)
    with pytest.raises(ValueError):
        plan.refine(*args, w=w, want=("info", "K"))
    for kw in (dict(max_rounds=-1), dict(max_rounds=17), dict(prim_tol=-1.0),
               dict(dual_tol=float("nan")), dict(face_tol=float("inf"))):
        with pytest.raises(CmpcError, match="cmpc_refine_run"):
            plan.refine(*args, w=w, **kw)
    ok = plan.refine(*args, w=w, max_rounds=16, prim_tol=1e-8, dual_tol=1e-8, face_tol=1e-6)
    torch.cuda.synchronize(plan.device)
    assert set(ok) == {"info", "res"} and np.all(ok["info"].cpu().numpy() == 0)


def test_repeatable_and_position_independent(plan):
    """6. Twice, reversed, permuted, B = 1, and tiled past one grid-stride pass (8192 blocks)."""
    case, _ = _fixture(plan, "qp_terrain.npz", "_A")
    B = len(case["w"])
    a, b = _refine(plan, case), _refine(plan, case)
    assert all(np.array_equal(a[n], b[n]) for n in ALL)
    rev = {k: (v[::-1].copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    r = _refine(plan, rev)
    assert all(np.array_equal(r[n][::-1], a[n]) for n in ALL)
    perm = np.random.default_rng(1).permutation(B)
    p = _refine(plan, case, idx=perm)
    assert all(np.array_equal(p[n], a[n][perm]) for n in ALL)
    one = _refine(plan, case, idx=np.array([B - 3]))
    assert all(np.array_equal(one[n][0], a[n][B - 3]) for n in ALL)
    reps = 8192 // B + 2
    big = _refine(plan, {k: np.tile(v, (reps,) + (1,) * (v.ndim - 1)) for k, v in case.items()
                         if isinstance(v, np.ndarray)})
    assert all(np.array_equal(big[n], np.tile(a[n], (reps,) + (1,) * (a[n].ndim - 1))) for n in ALL)


def _end_to_end_batch():
    """synth.make_config(2, B=64) plus the four qp_hard instances."""
    from cmpc import synth
    batch = synth.make_config(2, B=64)
    hard = load_fixture("qp_hard.npz")
    return {k: np.concatenate([np.asarray(batch[k]), np.asarray(hard[k]).astype(batch[k].dtype)])
            for k in IN}


def test_end_to_end_solve_then_refine(plan):
    """7. 68 instances solved with default parameters, then refined in place."""
    from cmpc import to_device_batch
    from oracle import active_set
    batch = _end_to_end_batch()
    d = to_device_batch(batch, plan.device)
    args = [d[k] for k in IN]
    w, st, it = plan.solve(*args)
    torch.cuda.synchronize(plan.device)
    w_in, st_in = w.cpu().numpy().copy(), st.cpu().numpy().copy()
    out = plan.refine(*args, w=w, w_out=w, status=st, want=ALL)
    torch.cuda.synchronize(plan.device)
    dev = {n: t.cpu().numpy() for n, t in out.items()}
    w_new, st_new = w.cpu().numpy(), st.cpu().numpy()
    B, N = len(w_in), plan.params.N
    cert = dev["info"] >= 0
    print("certified", int(cert.sum()), "of", B, "; info",
          dict(zip(*np.unique(dev["info"], return_counts=True))), "; status in",
          dict(zip(*np.unique(st_in, return_counts=True))), "; max res[2] over certified",
          float(dev["res"][cert, 2].max()) if cert.any() else None)
    assert np.all(dev["info"] != -1)
    assert np.array_equal(st_new, np.where(cert, 1, st_in))
    assert np.array_equal(w_new[~cert].view(np.uint32), w_in[~cert].view(np.uint32))
    assert np.array_equal(w_new[cert], dev["w64"][cert].astype(np.float32))
    U_in = w_in[:, 12 * N:].astype(np.float64)
    dist = np.abs(dev["w64"][:, 12 * N:] - U_in).max(1) / np.maximum(1.0, np.abs(U_in).max(1))
    assert np.allclose(dev["res"][:, 2], dist, rtol=1e-12, atol=0)
    # (a) against certify_batch_item on the float64 batch (the device received its fp32
    # rounding): the project's device-against-oracle bar, 1e-4 x max|u| (test_gpu_parity.TOL_U);
    # (b) against the same oracle on exactly the device's inputs, the fp32 arrays and the plan's
    # fp32 constants widened: the model's 1e-10 plus the device's 1e-8
    case = {k: d[k].cpu().numpy() for k in IN}
    case["w"] = w_in
    worst, worst_same = 0.0, 0.0
    for i in np.flatnonzero(cert):
        r = active_set.certify_batch_item(batch, i, w_in[i].astype(np.float64))
        assert max(r["kkt"].values()) <= active_set.CERT_TOL, (i, r["kkt"])
        uo = np.asarray(r["w"], np.float64)[12 * N:]
        worst = max(worst, float(np.abs(dev["w64"][i, 12 * N:] - uo).max() / np.abs(uo).max()))
        _, us = _oracle_u(case, i, plan.params, N)
        worst_same = max(worst_same,
                         float(np.abs(dev["w64"][i, 12 * N:] - us).max() / np.abs(us).max()))
    print("worst |w64 forces - certified optimum| / max|u| over certified rows: float64 batch",
          worst, "; the device's fp32 inputs", worst_same)
    assert worst <= 1e-4
    assert worst_same <= TOL + refine_util.ORACLE_REL


def test_solve_then_refine_in_a_captured_graph(plan):
    """8. A solve followed by a refine captured in one graph on a side stream; replayed twice with
    the inputs changed in place, each replay equals the eager calls."""
    from cmpc import synth, to_device_batch
    B, N = 8, plan.params.N
    batches = [synth.make_config(2, B=B), synth.next_tick(synth.make_config(2, B=B)),
               synth.make_batch(B, seed=5, mixed=True)]
    d = to_device_batch(batches[0], plan.device)
    args = [d[k] for k in IN]
    outs = (torch.empty((B, 24 * N), dtype=torch.float32, device=plan.device),
            torch.empty(B, dtype=torch.int32, device=plan.device),
            torch.empty(B, dtype=torch.int32, device=plan.device))
    ref = {"info": torch.empty(B, dtype=torch.int32, device=plan.device),
           "res": torch.empty((B, 3), dtype=torch.float64, device=plan.device),
           "w64": torch.empty((B, 24 * N), dtype=torch.float64, device=plan.device)}

    def step(stream=None):
        plan.solve(*args, out=outs, stream=stream)
        plan.refine(*args, w=outs[0], w_out=outs[0], status=outs[1], want=tuple(ref), out=ref,
                    stream=stream)

    def snapshot():
        torch.cuda.synchronize(plan.device)
        return [t.clone() for t in outs[:2]] + [t.clone() for t in ref.values()]

    step()                                                # (eager once, as ClosedLoop.capture does)
    torch.cuda.synchronize(plan.device)
    side = torch.cuda.Stream(plan.device)
    side.wait_stream(torch.cuda.current_stream(plan.device))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step(side)
    torch.cuda.current_stream(plan.device).wait_stream(side)
    seen = []
    for nb in batches[1:]:
        nd = to_device_batch(nb, plan.device)
        for k in IN:
            d[k].copy_(nd[k])
        graph.replay()
        replayed = snapshot()
        step()
        eager = snapshot()
        assert all(torch.equal(a, b) for a, b in zip(replayed, eager))
        assert torch.all(replayed[2] != -1) and torch.all(torch.isfinite(replayed[4]))
        seen.append(replayed[4])
    assert not torch.equal(seen[0], seen[1])              # the replays read the changed inputs
