"""GPU parity: the HIP solver vs the KKT-certified float64 optimum (oracle/tight_solver.py)
on the committed fixtures, plus size-independent properties at the benchmark sizes.

Tolerance (BASELINE.json north_star): contact-force primal within 1e-4 relative,
max_k,leg |U_gpu - U*| / max |U*| <= 1e-4 per instance.
"""
import numpy as np
import pytest
import torch

from parity_util import (load_fixture, fixture_batch, rel_err_U, split_w, rollout64,
                         feasibility, assert_verified)

pytestmark = pytest.mark.gpu
TOL_U = 1e-4


@pytest.mark.parametrize("name", ["qp_cfg1.npz", "qp_cfg2.npz"])
def test_fixture_parity(plan, name):
    from cmpc import solve_batch
    fx = load_fixture(name)
    batch = fixture_batch(fx)
    w, st, it = solve_batch(batch, plan=plan)
    err = rel_err_U(w, fx["w"])
    assert np.all(st == 1), (st, it)
    assert err.max() <= TOL_U, (err.max(), int(err.argmax()))
    # X is the rollout of U under the same dynamics (the equality rows of the reference QP)
    Xg, Ug = split_w(w.astype(np.float64))
    Xr = rollout64(batch, Ug)
    assert np.max(np.abs(Xg - Xr)) < 1e-4
    assert feasibility(batch, Ug).max() < 1e-3


def test_hard_cases(plan):
    """Benchmark-batch instances that exposed solver weaknesses (tests/golden/make_golden.py
    HARD_CASES: a degenerate vertex, an ill-conditioned face set, wandering repairs), each
    replicated past the latency-mode threshold (B > 4 x CUs) so they run the same arithmetic
    as in the 65,536-instance batch they came from."""
    from cmpc import solve_batch
    fx = load_fixture("qp_hard.npz")
    reps = 1100
    batch = {k: np.repeat(v, reps, axis=0) for k, v in fixture_batch(fx).items()}
    w, st, it = solve_batch(batch, plan=plan)
    assert np.all(st == 1), [(tuple(c), np.unique(st[i * reps:(i + 1) * reps]).tolist())
                             for i, c in enumerate(fx["cases"])]
    err = rel_err_U(w, np.repeat(fx["w"], reps, axis=0))
    assert err.max() <= TOL_U, (err.max(), int(err.argmax()) // reps)
    assert it.max() < 400, [int(it[i * reps:(i + 1) * reps].max()) for i in range(len(fx["w"]))]


def test_status_and_iters_sane(plan):
    from cmpc import solve_batch, synth
    b = synth.make_config(2, B=4096)
    w, st, it = solve_batch(b, plan=plan)
    assert np.all(np.isfinite(w))
    assert np.all(st == 1), np.unique(st, return_counts=True)
    Xg, Ug = split_w(w.astype(np.float64))
    assert feasibility(b, Ug).max() < 1e-2
    assert np.max(np.abs(Xg - rollout64(b, Ug))) < 1e-3


def _bins(contact):
    nf = 3 * (contact != 0).reshape(contact.shape[0], -1).sum(1)
    return np.searchsorted(np.array([96, 128, 144, 160, 192]), nf)


def test_heaviest_bin_parity(plan):
    """64 certified instances with more than 160 free forces (the NC = 192 bin,
    tests/golden/qp_nc192.npz), solved as one small batch (latency mode) and replicated 20x past
    the latency threshold (throughput mode, the arithmetic of a 65,536 batch)."""
    from cmpc import solve_batch
    fx = load_fixture("qp_nc192.npz")
    batch = fixture_batch(fx)
    assert np.all(_bins(batch["contact"]) == 4)
    w, st, it = solve_batch(batch, plan=plan)
    assert np.all(st == 1), (st, it)
    err = rel_err_U(w, fx["w"])
    assert err.max() <= TOL_U, (err.max(), int(err.argmax()))
    reps = 20
    big = {k: np.repeat(v, reps, axis=0) for k, v in batch.items()}
    w, st, it = solve_batch(big, plan=plan)
    assert np.all(st == 1)
    err = rel_err_U(w, np.repeat(fx["w"], reps, axis=0))
    assert err.max() <= TOL_U, (err.max(), int(err.argmax()) // reps)


def _tight(batch, i):
    from oracle import mpc_qp, tight_solver
    qp = mpc_qp.build_qp(batch["Ad"][i], batch["Bd"][i], batch["gd"][i], batch["x0"][i],
                         batch["xref"][i].T, batch["contact"][i])
    r = tight_solver.solve(qp)
    assert max(r["kkt"].values()) < 1e-8
    return r["w"]


def test_edge_contact_patterns(plan):
    """All-swing (no free force), all-stance (192 free forces, largest bin), single foot."""
    from cmpc import solve_batch, synth
    b = synth.make_config(2, B=6)
    b["contact"][0] = 0
    b["contact"][1] = 1
    b["contact"][2] = 0
    b["contact"][2, 1] = 1
    b["contact"][3] = 0
    b["contact"][3, :, ::2] = 1
    w, st, it = solve_batch(b, plan=plan)
    assert np.all(st == 1), st
    Xg, Ug = split_w(w.astype(np.float64))
    assert np.all(Ug[0] == 0)
    assert np.max(np.abs(Xg[0] - rollout64(b, Ug)[0])) < 1e-4
    for i in range(4):
        wr = _tight(b, i)
        assert rel_err_U(w[i:i + 1], wr[None])[0] <= TOL_U


def test_shorter_horizon_plan():
    from cmpc import Plan, SolverParams, solve_batch, synth
    p = Plan(SolverParams(N=8, max_batch=16))
    b = synth.make_batch(5, seed=11, mixed=True, N=8)
    w, st, it = solve_batch(b, plan=p)
    assert w.shape == (5, 24 * 8) and np.all(st == 1)
    for i in range(5):
        assert rel_err_U(w[i:i + 1], _tight(b, i)[None], N=8)[0] <= TOL_U


def test_short_horizons():
    """Horizons N = 1 and 5 (below 16 and no power of two), where the gradient scans'
    `(1 << l) >= N` cut and the `c < N` masks decide (cmpc_gradient.h gradient): the nilpotent
    step matrix as generated and the attitude-damped one of test_general_step_matrix, each with
    team mode forced and off.  Every instance is verified and within 1e-4 of its certified
    optimum."""
    from cmpc import Plan, SolverParams, solve_batch, synth
    keys = ("Ad", "Bd", "gd", "x0", "xref", "contact")
    for N in (1, 5):
        b = synth.make_batch(8, seed=11, mixed=True, N=N)
        for damped in (False, True):
            if damped:
                for r in range(3, 6):
                    b["Ad"][:, r, r] = 0.999
            ref = np.stack([_tight(b, i) for i in range(8)])
            for team in (1 << 40, 0):
                p = Plan(SolverParams(N=N, max_batch=16))
                p.set_team(team)
                w, st, it = solve_batch({k: b[k] for k in keys}, plan=p)
                err = rel_err_U(w, ref, N=N)
                print("N", N, "damped", damped, "team", team != 0, "status", st.tolist(),
                      "iters", it.tolist(), "max rel err", float(err.max()))
                assert np.all(st == 1), (N, damped, team, st.tolist())
                assert err.max() <= TOL_U, (N, damped, team, float(err.max()))


def test_deterministic(plan):
    from cmpc import solve_batch, synth
    b = synth.make_config(2, B=512)
    w1, s1, i1 = solve_batch(b, plan=plan)
    w2, s2, i2 = solve_batch(b, plan=plan)
    assert np.array_equal(w1, w2) and np.array_equal(s1, s2) and np.array_equal(i1, i2)


@pytest.mark.parametrize("cfg", [3, 2])
def test_instance_order_independent(plan, cfg):
    """Each instance is one independent solve (centroidal_mpc.py:69-120): its answer must not
    depend on which instances its wave solved before it.  The batch (16,384 instances: every
    bin, the one-wave persistent kernels) is solved, then solved again with the instances in a
    random order, so that each instance lands at another queue position, on another wave, after
    other instances; the outputs, put back in order, are bitwise equal per instance.  (Round 5's
    3-downdate-cap build failed this: state read from a previous instance.)"""
    from cmpc import solve_batch, synth
    b = synth.make_config(cfg, B=16384)
    keys = ("Ad", "Bd", "gd", "x0", "xref", "contact")
    w0, s0, i0 = solve_batch(b, plan=plan)
    perm = np.random.default_rng(6).permutation(16384)
    w1, s1, i1 = solve_batch({k: b[k][perm] for k in keys}, plan=plan)
    inv = np.argsort(perm)
    w1, s1, i1 = w1[inv], s1[inv], i1[inv]
    same = np.all(w0.view(np.uint32) == w1.view(np.uint32), axis=1) & (s0 == s1) & (i0 == i1)
    assert same.all(), (int((~same).sum()), np.flatnonzero(~same)[:8].tolist())


def test_class_order_independent():
    """cmpc_plan_set_heavy_first: which register class is submitted first changes only where
    and when each instance runs, never its result (one wave solves it, deterministically).
    Both orders on a config-3 batch above the team bound, bitwise."""
    from cmpc import Plan, SolverParams, solve_batch, synth
    b = synth.make_config(3, B=8192)
    p = Plan(SolverParams(max_batch=8192))
    assert p.heavy_first_batch() > 0
    out = []
    for hmin in (0, 1):  # never / always
        p.set_heavy_first(hmin)
        assert p.heavy_first_batch() == hmin
        out.append(solve_batch(b, plan=p))
    p.set_heavy_first(-1)
    (w0, s0, i0), (w1, s1, i1) = out
    assert np.all(s0 == 1)
    assert np.array_equal(w0, w1) and np.array_equal(s0, s1) and np.array_equal(i0, i1)


def test_plan_stats(plan):
    """cmpc_plan_stats (ABI 6, include/cmpc.h): the acceptance counters start at zero after a
    reset, count the same events when the same batch is solved again (the solver is
    deterministic), and a certified-bound miss is always an answer returned as status 2."""
    from cmpc import solve_batch, synth
    b = synth.make_config(3, B=16384)
    plan.stats(reset=True)
    assert plan.stats() == {"loose": 0, "status2_cert": 0, "guard_refactors": 0}
    _, s0, _ = solve_batch(b, plan=plan)
    a = plan.stats(reset=True)
    _, s1, _ = solve_batch(b, plan=plan)
    assert plan.stats(reset=True) == a
    assert np.array_equal(s0, s1)
    assert min(a.values()) >= 0 and a["loose"] + a["guard_refactors"] > 0, a
    assert a["status2_cert"] <= int((s0 == 2).sum()), (a, int((s0 == 2).sum()))


def test_full_size_certified_sample(plan):
    """The full config-3 batch (65,536 trot + mixed, the headline workload) in one solve: every
    instance solved and feasible -- status 1 but for at most a 1e-4 fraction at status 2 (a
    point that missed the certified face bound, include/cmpc.h) --, X the rollout of U, and 512
    instances stratified over the
    bins (tests/golden/qp_cfg3.npz: 128 / 256 / 87 / 40 / 1 at NC 96 / 128 / 144 / 160 / 192 --
    drawn as 128 / 256 / 127 / 1 over round 1's four bins, whose NC 160 bin now splits into two)
    within 1e-4 of their KKT-certified optimum."""
    from cmpc import solve_batch, synth
    from parity_util import input_digest
    fx = load_fixture("qp_cfg3.npz")
    b = synth.make_config(3, B=65536)
    idx = fx["idx"]
    assert input_digest(b, idx) == str(fx["digest"]), "config-3 generator drifted"
    assert np.array_equal(np.bincount(_bins(b["contact"][idx]), minlength=5), [128, 256, 87, 40, 1])
    w, st, it = solve_batch(b, plan=plan)
    assert np.all(np.isfinite(w))
    ok = assert_verified(st)
    Xg, Ug = split_w(w.astype(np.float64))
    assert feasibility(b, Ug).max() < 1e-2
    sub = {k: b[k][idx] for k in ("Ad", "Bd", "gd", "x0")}
    assert np.max(np.abs(Xg[idx] - rollout64(sub, Ug[idx]))) < 1e-3
    err = rel_err_U(w[idx], fx["w"])
    err1 = np.where(ok[idx], err, 0.0)   # status 1: the parity bar; status 2: no 1e-4 promise
    worst = int(err1.argmax())
    assert err1.max() <= TOL_U, (err1.max(), int(idx[worst]), int(fx["bins"][worst]))
    assert err.max() <= 10 * TOL_U, (err.max(), int(idx[err.argmax()]))


def test_check_termination_reference_interval():
    """OPTS check_termination = 10 (centroidal_mpc.py:31, cmpc_params.check_termination): the
    termination test (polish trigger) runs only every 10th ADMM iteration.  Same solutions within
    the parity bar; every cold solve ends at a multiple of 10 iterations.  Both the small-batch
    (team) and the large-batch path."""
    from cmpc import Plan, SolverParams, solve_batch
    fx = load_fixture("qp_cfg2.npz")
    plan10 = Plan(SolverParams(max_batch=4096, check_termination=10))
    for reps in (1, 40):
        batch = {k: np.repeat(v, reps, axis=0) for k, v in fixture_batch(fx).items()}
        w, st, it = solve_batch(batch, plan=plan10)
        assert np.all(st == 1), np.unique(st, return_counts=True)
        assert np.all(it % 10 == 0) and it.min() >= 10, np.unique(it)
        err = rel_err_U(w, np.repeat(fx["w"], reps, axis=0))
        assert err.max() <= TOL_U, err.max()


@pytest.mark.parametrize("reps", [1, 1100])
def test_general_step_matrix(plan, reps):
    """A step matrix that is NOT I + N with N^2 = 0 takes the general condensation and the
    gradient's squared powers of A (the reference's nilpotent ZOH takes the closed forms,
    cmpc_condense.h condense_tiles_nil): a perturbed Ad (an attitude-damping term on the Euler
    rates, A[3:6, 3:6] = 0.999 I) is solved to 1e-4 of ITS certified optimum, in latency mode and
    replicated past the latency threshold (throughput mode)."""
    from cmpc import solve_batch, synth
    b = synth.make_config(2, B=8)
    for i in range(8):
        for r in range(3, 6):
            b["Ad"][i, r, r] = 0.999
    Nm = b["Ad"][0].astype(np.float32) - np.eye(12, dtype=np.float32)
    assert np.any(Nm @ Nm != 0)  # not nilpotent: the general path
    big = {k: np.repeat(v, reps, axis=0) for k, v in b.items() if isinstance(v, np.ndarray)
           and v.shape[:1] == (8,)}
    w, st, it = solve_batch(big, plan=plan)
    assert np.all(st == 1), np.unique(st, return_counts=True)
    for i in range(8):
        wr = _tight(b, i)
        assert rel_err_U(w[i * reps:i * reps + 1], wr[None])[0] <= TOL_U, i


def test_general_step_matrix_one_wave_latency():
    """The same eight damped instances (free-force counts 96 .. 150: bins NC 96, 128, 144, 160)
    with team mode off: a small batch then runs one wave per QP in latency mode, where the NC 96 /
    128 kernel condenses a general A by the block-row form (cmpc_condense.h condense_tiles_bc), which
    the default team rule never reaches.  Both group kernels must be the ones launched.  The
    small-batch rule of parity_util.assert_verified (at most one status 2) and test_gpu_terrain's
    bars: status 1 within 1e-4 of the certified optimum, status 2 within 1e-3."""
    from cmpc import Plan, SolverParams, solve_batch, synth
    b = synth.make_config(2, B=8)
    for r in range(3, 6):
        b["Ad"][:, r, r] = 0.999
    Nm = b["Ad"][0].astype(np.float32) - np.eye(12, dtype=np.float32)
    assert np.any(Nm @ Nm != 0)
    p = Plan(SolverParams(max_batch=16))
    p.set_team(0)
    names = p.solve_kernels(8)
    assert names[0] and names[1] and all("group" in k for k in names[:2]), names
    w, st, it = solve_batch({k: b[k] for k in ("Ad", "Bd", "gd", "x0", "xref", "contact")}, plan=p)
    print("status", st.tolist(), "iters", it.tolist())
    ok = assert_verified(st)
    errs = [rel_err_U(w[i:i + 1], _tight(b, i)[None])[0] for i in range(8)]
    print("rel err", errs)
    for i in range(8):
        assert errs[i] <= (TOL_U if ok[i] else 1e-3), (i, int(st[i]), errs[i])


def test_general_step_matrix_heavy_bins(plan):
    """The general-A path (the squared-power gradient scans and forward condensation, fp32
    rollout) on the NC 144 / 160 / 192 kernels and the hard instances (face-downdate repairs):
    the attitude-damped Ad of test_general_step_matrix on the cfg2 fixtures' heavier instances,
    16 of the NC 192 fixtures and the four hard cases, replicated past the small-batch bound so
    that the one-wave group kernels run them.  Every instance is certified on the CPU against
    its own KKT-certified optimum (oracle/active_set.py, seeded by the GPU's answer).  A general
    A keeps the relative multiplier test: a loose acceptance there is status 2."""
    from cmpc import solve_batch
    from oracle import active_set, mpc_qp
    keys = ("Ad", "Bd", "gd", "x0", "xref", "contact")
    c2, c192, hd = load_fixture("qp_cfg2.npz"), load_fixture("qp_nc192.npz"), load_fixture("qp_hard.npz")
    heavy = np.flatnonzero(3 * (c2["contact"] != 0).reshape(len(c2["contact"]), -1).sum(1) > 128)[:12]
    b = {k: np.concatenate([c2[k][heavy], c192[k][:16], hd[k]]).astype(np.float64) for k in keys}
    for r in range(3, 6):
        b["Ad"][:, r, r] = 0.999
    B0, reps = len(b["Ad"]), 96
    big = {k: np.repeat(v, reps, axis=0) for k, v in b.items()}
    w, st, it = solve_batch(big, plan=plan)
    assert np.mean(st == 1) > 0.99 and np.all((st == 1) | (st == 2)), np.unique(st, return_counts=True)
    for i in range(B0):
        qp = mpc_qp.build_qp(b["Ad"][i], b["Bd"][i], b["gd"][i], b["x0"][i], b["xref"][i].T,
                             b["contact"][i])
        wi = w[i * reps].astype(np.float64)
        r = active_set.certified_optimum(qp, wi)
        assert max(r["kkt"].values()) <= active_set.CERT_TOL, i
        errs = rel_err_U(w[i * reps:(i + 1) * reps], np.repeat(r["w"][None], reps, axis=0))
        ok = st[i * reps:(i + 1) * reps] == 1
        assert errs[ok].max() <= TOL_U, (i, errs.max())
