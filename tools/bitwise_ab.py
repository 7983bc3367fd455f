"""A/B of two library builds for bit-identical results: solve the headline batch (config 3,
65,536) cold and its next tick warm, config 2 at 4,096 cold, and small batches that walk the
paths those miss (small_cases), with the library given, and write (w, status, iterations, and
y / lam where a case returns them, and what Plan.kkt, Plan.gain, Plan.vjp and Plan.refine make of
four of the small batches where the library has those entries: evaluate); run once per library
in separate processes, then compare.
    python tools/bitwise_ab.py LIB OUT.npz            (GPU)
    python tools/bitwise_ab.py --compare A.npz B.npz   (CPU)"""
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "convex-mpc-unitree-go2_amd"))


GOLDEN = REPO / "tests" / "golden"
KEYS = ("Ad", "Bd", "gd", "x0", "xref", "contact")


def small_cases(res):
    """Batches of at most ~1,000 instances, seconds each: team mode forced, cmpc_solve_ref, per-robot
    terrain (one invalid row) and weights, a primal-only warm start, an all-swing instance, N = 8,
    a general step matrix in every mode (general_cases: the fixtures above are all nilpotent), and
    the evaluation entries on four of those solves (evaluate)."""
    import torch
    from cmpc import Plan, SolverParams, _lib, to_device_batch, synth

    def put(tag, r, extra=()):
        torch.cuda.synchronize()
        for k, v in zip(("w", "st", "it") + tuple(extra), r):
            res[f"{tag}_{k}"] = v.cpu().numpy()
        return r

    def dev(np_batch):
        return to_device_batch({k: np.ascontiguousarray(np_batch[k]) for k in KEYS})

    def args(d):
        return tuple(d[k] for k in KEYS)

    def f32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    def evaluate(tag, p, d, r, **kw):
        """On the batch d solved with lam_out as r (kw: its per-robot values): Plan.kkt with lam
        given and recovered; Plan.gain with every output, faces read off w and then given;
        Plan.vjp of a seeded gw the same two ways, and x0's gradient asked for alone (it must not
        depend on what else is asked); Plan.refine with every output, w_out and status, faces
        read off w, all-zero masks given next to w (no face held: the repair rounds run), and
        max_rounds = 0."""
        out, w, lam = {}, r[0], r[3]
        if hasattr(p.lib, "cmpc_kkt_run"):
            out["kkt_given"] = p.kkt(*args(d), w, lam=lam, **kw)
            out["kkt_recovered"] = p.kkt(*args(d), w, **kw)
        if hasattr(p.lib, "cmpc_gain_run"):
            g = p.gain(*args(d), w=w, want=_lib.GAIN_OUTPUTS, **kw)
            out.update({f"gain_w_{k}": v for k, v in g.items()})
            g = p.gain(*args(d), faces=g["faces"], want=_lib.GAIN_OUTPUTS, **kw)
            out.update({f"gain_faces_{k}": v for k, v in g.items()})
            held = g["faces"]
        if hasattr(p.lib, "cmpc_vjp_run"):
            gw = f32(np.random.default_rng(7).standard_normal(tuple(w.shape)))
            for mode, sel in (("w", dict(w=w)), ("faces", dict(faces=held))):
                g = p.vjp(*args(d), gw, want=_lib.VJP_OUTPUTS, **sel, **kw)
                out.update({f"vjp_{mode}_{k}": v for k, v in g.items()})
            out["vjp_x0_alone"] = p.vjp(*args(d), gw, w=w, want=("x0",), **kw)["x0"]
        if hasattr(p.lib, "cmpc_refine_run"):
            for mode, sel in (("w", dict(w=w)), ("free", dict(w=w, faces=torch.zeros_like(held))),
                              ("check", dict(w=w, max_rounds=0))):
                wo = w.clone()
                st = torch.zeros(len(w), dtype=torch.int32, device=w.device)
                g = p.refine(*args(d), **dict(dict(max_rounds=8), **sel), w_out=wo, status=st,
                             want=_lib.REFINE_OUTPUTS, **kw)
                out.update({f"refine_{mode}_{k}": v for k, v in g.items()})
                out.update({f"refine_{mode}_w_out": wo, f"refine_{mode}_status": st})
        torch.cuda.synchronize()
        res.update({f"{tag}_{k}": v.cpu().numpy() for k, v in out.items()})

    plan = Plan(SolverParams(max_batch=4096))
    d = dev(np.load(GOLDEN / "qp_cfg1.npz"))
    evaluate("cfg1_ref", plan, d, put("cfg1_ref", plan.solve(*args(d), lam_out=True), ("lam",)))
    # team mode forced, on the fixtures of every bin (y out: the dual writer in team mode)
    plan.set_team(1 << 40)
    for name in ("qp_cfg1", "qp_nc192", "qp_hard"):
        put("team_" + name, plan.solve(*args(dev(np.load(GOLDEN / f"{name}.npz"))), y_out=True), ("y",))
    plan.set_team(-1)
    # cmpc_solve_ref on the certified next-tick subset: lam out, then w_init + lam_init in
    idx = np.load(GOLDEN / "qp_next_tick.npz")["idx"]
    b1 = synth.make_config(2, B=4096)
    b2 = synth.next_tick(b1)
    d1 = dev({k: b1[k][idx] for k in KEYS})
    d2 = dev({k: b2[k][idx] for k in KEYS})
    r1 = plan.solve(*args(d1), lam_out=True)
    put("ref_tick0", r1, ("lam",))
    put("ref_tick1", plan.solve(*args(d2), w_init=r1[0], lam_init=r1[3], lam_out=True), ("lam",))
    # a primal-only warm start (w_init without duals), y out
    put("warm_primal", plan.solve(*args(d2), w_init=r1[0], y_out=True), ("y",))
    # per-robot mu / fz_min, one invalid row (status -10); per-robot Q / R, one invalid row
    ft = np.load(GOLDEN / "qp_terrain.npz")
    mu, fz = ft["mu_A"].copy(), ft["fz_min_A"].copy()
    mu[3] = -1.0
    d, kw = dev(ft), dict(mu=f32(mu), fz_min=f32(fz))
    evaluate("terrain", plan, d, put("terrain", plan.solve(*args(d), lam_out=True, **kw), ("lam",)), **kw)
    fw = np.load(GOLDEN / "qp_weights.npz")
    put("weights", plan.solve(*args(dev(fw)), Q=f32(fw["Q_A"]), R=f32(fw["R_A"]), y_out=True), ("y",))
    R = fw["R_B"].copy()
    R[5, 2] = 0.0
    d, kw = dev(fw), dict(Q=f32(fw["Q_B"]), R=f32(R))
    evaluate("weights_bad_row", plan, d,
             put("weights_bad_row", plan.solve(*args(d), lam_out=True, **kw), ("lam",)), **kw)
    # an all-swing instance among stance ones
    fc = {k: np.load(GOLDEN / "qp_cfg1.npz")[k].copy() for k in KEYS}
    fc["contact"][1] = 0
    put("all_swing", plan.solve(*args(dev(fc)), lam_out=True), ("lam",))
    # a plan with N = 8
    p8 = Plan(SolverParams(N=8, max_batch=1024))
    d = dev(synth.make_batch(768, seed=11, mixed=True, N=8))
    put("n8", p8.solve(*args(d), y_out=True), ("y",))
    evaluate("n8_ref", p8, d, put("n8_ref", p8.solve(*args(d), lam_out=True), ("lam",)))
    general_cases(plan, put, dev, args)


def damped(b):
    """The attitude-damped step matrix of tests/test_gpu_parity.py::test_general_step_matrix: not
    I + N with N^2 = 0, so the solve takes the general condensations and gradient."""
    b = {k: np.array(b[k], dtype=np.float64) for k in KEYS}
    for r in range(3, 6):
        b["Ad"][:, r, r] = 0.999
    return b


def general_cases(plan, put, dev, args):
    """General (non-nilpotent) step matrix, every bin.  Team forced: the team kernel's general
    branch.  Team off at B <= 4 x CUs: latency mode, block-row condensation on NC 96 / 128 and
    forward condensation on the heavier bins.  gen_heavy x 40 (1,280 > 4 x CUs) under the default
    rule: throughput mode, forward condensation everywhere, plain sweep on NC 144 / 160 / 192."""
    from cmpc import synth
    # free-force counts 96, 105, 120, 150, 126, 132, 147, 96: bins NC 96, 128, 144 and 160, with
    # partial last pivot blocks (105 -> 27 pivot groups, 150 -> 38)
    gen8 = damped(synth.make_config(2, B=8))
    # test_general_step_matrix_heavy_bins' 32 instances: 12 cfg2 fixtures with n in 129..150, 16
    # of qp_nc192.npz (n 162 / 165) and the 4 of qp_hard.npz
    c2, c192, hd = (np.load(GOLDEN / f"{f}.npz") for f in ("qp_cfg2", "qp_nc192", "qp_hard"))
    heavy = np.flatnonzero(3 * (c2["contact"] != 0).reshape(len(c2["contact"]), -1).sum(1) > 128)[:12]
    gen_heavy = damped({k: np.concatenate([c2[k][heavy], c192[k][:16], hd[k]]) for k in KEYS})
    for tag, b, modes in (("gen8", gen8, (("team", 1 << 40, 1), ("wave", 0, 1), ("auto", -1, 1))),
                          ("gen_heavy", gen_heavy, (("team", 1 << 40, 1), ("wave", 0, 1), ("x40", -1, 40)))):
        for mode, team, reps in modes:
            plan.set_team(team)
            d = dev({k: np.repeat(b[k], reps, axis=0) for k in KEYS})
            put(f"{tag}_{mode}", plan.solve(*args(d), y_out=True), ("y",))
    plan.set_team(-1)


def run(lib, out):
    import torch
    from cmpc import _lib
    _lib._lib = _lib.load(lib)
    from cmpc import Plan, SolverParams, to_device_batch, synth
    plan = Plan(SolverParams(max_batch=65536))
    res = {}
    for tag, b, prev in (("cfg3", synth.make_config(3), None),
                         ("cfg2", synth.make_config(2, B=4096), None),
                         ("cfg3_next_warm", synth.next_tick(synth.make_config(3)), synth.make_config(3))):
        kw = {}
        if prev is not None:
            dp = to_device_batch(prev)
            y = torch.empty((dp["Ad"].shape[0], 12 * 16), dtype=torch.float32, device=dp["Ad"].device)
            w0, _, _ = plan.solve(*(dp[k] for k in ("Ad", "Bd", "gd", "x0", "xref", "contact")), y_out=y)
            kw = dict(w_init=w0, y_init=y)
        d = to_device_batch(b)
        w, st, it = plan.solve(*(d[k] for k in ("Ad", "Bd", "gd", "x0", "xref", "contact")), **kw)
        torch.cuda.synchronize()
        res[tag + "_w"] = w.cpu().numpy()
        res[tag + "_st"] = st.cpu().numpy()
        res[tag + "_it"] = it.cpu().numpy()
    small_cases(res)
    np.savez_compressed(out, **res)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    ok = True
    if sorted(A.files) != sorted(B.files):
        print("the two files hold different cases")
        ok = False
    for k in sorted(set(A.files) & set(B.files)):
        # the arrays' bytes: equal NaN bit patterns (an invalid row's results) are equal
        x, y = (np.ascontiguousarray(v[k]).reshape(len(v[k]), -1).view(np.uint8) for v in (A, B))
        same = A[k].dtype == B[k].dtype and x.shape == y.shape and bool(np.all(x == y))
        nd = int(np.any(x != y, axis=1).sum()) if x.shape == y.shape else "all"
        print(f"{k}: {'bit-identical' if same else f'{nd} instances differ'}")
        ok = ok and same
    print("ALL BIT-IDENTICAL" if ok else "DIFFERENT")


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        run(sys.argv[1], sys.argv[2])
