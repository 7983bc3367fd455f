"""The ADMM iteration itself -- iterates, rho adaptation, exit status, the unpolished outputs and
the solver knobs -- against the float64 reference of the documented iteration (tests/admm_ref.py;
include/cmpc.h states the same definitions).  Every other GPU test ends in the active-set polish,
which re-solves the QP on the face set ADMM hands it: those tests see a wrong iteration only as
more iterations.

The polish is switched off by polish_stable = max_iter + 1: a session starts only after the face
set stayed unchanged for polish_stable iterations, and the run has fewer, so the trigger can
never fire and the instance returns ADMM's z, y and the status of the residual test at
iters == max_iter.

Batches (admm_ref.batches(), at most 22 instances): `main` = test_gpu_admm_passes.batch(16)
(n = 24 .. 129 with the rho boundary 96 / 99, the tile edges 126 / 129, the step tables with empty
and full steps) and two instances each of n = 147, 162, 192 (NC 160, NC 192); `s5`, `s1` = the
step tables at horizons 5 and 1.  Every run is made by the wave kernels (team mode off) and by the
team kernel (team mode forced), on Plan(SolverParams(max_batch=64, ...)).

Bars (tests/test_admm_ref.py sets and asserts them on the CPU): k iterations after the
factorization in use (k = max_iter unless rho changed, admm_ref.since_refactor) the forces are
within 4 D_k x S of z_k, S = max(1, max|z_ref|), and y_out within 4 D_k x max(max|y_ref|, rho S)
plus four float32 roundings of max|q| of y_k, with D_k = admm_ref.D_K (2.0e-4, 8.2e-5, 9.2e-5,
3.5e-5, 8.4e-6, 1.0e-6 at k = 1, 2, 3, 5, 8, 30), the fp32 model's own deviation from the
reference.  alpha = 1.9 and rho = 1e-5 have tables of their own (admm_ref.D_OFF, with the reason):
at the default table the device measured up to 11 x (alpha = 1.9, k = 8) and 3.3 x (rho = 1e-5,
k = 8) the bar where the fp32 model itself stands at 14 x and 1.5 x; y_out at k = 30 measured
1.19 x without the rounding floor (an error of 4.4e-8 = one float32 rounding of |q| = 0.69), and
the second run of rho = 0.05 at (2, 9), one iteration after its last change of rho, 1.5 x at D_8.
lam_out is compared at the device's own u with the float64 evaluation of the header's formulas,
within 4 x 4.2e-5 of the instance's largest multiplier (the float32 NumPy evaluation's deviation
at the reference's z_k, admm_ref.LAM_D).

Measured worst ratios to the bar (MI355X; forces / y_out, the worst of the three batches):

    defaults       k      1          2          3          5          8          30
      wave            0.43/0.07  0.26/0.15  0.44/0.10  0.41/0.15  0.21/0.29  0.22/0.19
      team            0.44/0.07  0.51/0.20  0.45/0.09  0.44/0.15  0.65/0.29  0.25/0.22
    off default    k      1          3          8             (wave; team within 0.1 of it
      alpha = 1.0     0.43/0.11  0.45/0.18  0.93/0.34          except sigma = 0 at k = 8:
      alpha = 1.9     0.29/0.04  0.19/0.05  0.12/0.03          0.62/0.22)
      rho = 1e-5      0.29/0.12  0.28/0.16  0.27/0.18
      rho = 1e-3      0.06/0.01  0.08/0.01  0.51/0.11
      sigma = 0       0.34/0.07  0.27/0.09  0.27/0.22
      sigma = 1e-4    0.16/0.02  0.21/0.19  0.63/0.36
    rho adaptation (interval, max_iter): (2, 8) 0.01, (2, 9) 0.06, (3, 8) 0.01, (3, 9) 0.01
    lam_out: 0.03 (k = 1), 0.06 (k = 8), 0.14 (k = 30), both modes
    exit status: every verdict as the reference's, also on the two instances left out

Mutation checks (each one-line change of admm_iteration / solve_instance, built and run once by
hand): alpha fixed at 1.6f fails 12 tests of this file, sigma dropped from set_rho's shift 14,
kRhoLow false for NC = 128 28, `if (adapt || last)` reduced to `if (adapt)` 2
(test_exit_status[max_iter=30-eps_abs]), y updated from the old z 42.
"""
import numpy as np
import pytest

import admm_ref
from parity_util import load_fixture, split_w, rollout64
from test_gpu_admm_passes import batch, _check, MODES

pytestmark = pytest.mark.gpu
STATE_TOL = 1e-4        # states against the float64 rollout of the device's own forces
KNOBS = ([dict(alpha=v) for v in (1.0, 1.9)] + [dict(rho=v) for v in (1e-5, 1e-3)] +
         [dict(sigma=v) for v in (0.0, 1e-4)] + [dict(polish_stable=v) for v in (1, 6)] +
         [dict(polish_repairs=v) for v in (0, 1)] + [dict(adaptive_rho_interval=0)])


def _ids(sets):
    return ["-".join(f"{k}={v}" for k, v in s.items()) or "default" for s in sets]


def _solve(name, mode, max_iter, want="y", **params):
    """Batch `name` for max_iter iterations without a polish: (U (B, 12N) float64 forces,
    X (B, N, 12) states, status, iters, y_out or lam_out as float64)."""
    import torch
    from cmpc import Plan, SolverParams
    from cmpc.solver import to_device_batch
    N, b = admm_ref.batches()[name]
    plan = Plan(SolverParams(N=N, max_batch=64, max_iter=max_iter, polish_stable=max_iter + 1,
                             **params))
    plan.set_team(MODES[mode])
    d = to_device_batch({k: np.array(v) for k, v in b.items()}, plan.device)
    out = plan.solve(d["Ad"], d["Bd"], d["gd"], d["x0"], d["xref"], d["contact"],
                     **({"y_out": True} if want == "y" else {"lam_out": True}))
    torch.cuda.synchronize(plan.device)
    w, st, it, dual = (t.cpu().numpy() for t in out)
    plan.close()
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(dual))
    X, U = split_w(w.astype(np.float64), N)
    assert np.max(np.abs(X - rollout64(b, U))) < STATE_TOL
    return U.reshape(len(U), -1), X, st, it, dual.astype(np.float64)


def _compare(name, mode, k, only=None, **params):
    """One run against the reference: the worst ratios of the forces and of y_out to their bars
    over the instances `only` (None: all), after the exact checks."""
    refs = admm_ref.reference(name, k, **params)
    probs = admm_ref.batch_problems(name)
    U, X, st, it, y = _solve(name, mode, k, **params)
    worst = [0.0, 0.0]
    for i, (p, r) in enumerate(zip(probs, refs)):
        swing = np.ones(12 * p.N, bool)
        swing[p.idx] = False
        assert np.all(U[i][swing] == 0) and np.all(y[i][swing] == 0), (name, i)
        if r is None:      # no stance leg: nothing to iterate
            assert it[i] == 0 and st[i] == 1, (name, i, it[i], st[i])
            continue
        assert it[i] == k, (name, i, it[i])
        assert st[i] in (2, -2), (name, i, st[i])
        if only is not None and not only[i]:
            continue
        zr, yr = r["z"][-1], r["y"][-1]
        bar = admm_ref.bar(admm_ref.since_refactor(r), **params)
        S = max(1.0, float(np.max(np.abs(zr))))
        Sy = max(float(np.max(np.abs(yr))), r["rho"][-1] * S)
        floor = admm_ref.Y_FLOOR_ROUNDINGS * 2.0 ** -24 * float(np.max(np.abs(p.q)))
        eu = float(np.max(np.abs(U[i][p.idx] - zr))) / (bar * S)
        ey = float(np.max(np.abs(y[i][p.idx] - yr))) / (bar * Sy + floor)
        if max(eu, ey) > 1:
            print(f"  over the bar: {name}[{i}] n={p.n} k={k} {params} u {eu:.3g} y {ey:.3g}")
        worst = [max(worst[0], eu), max(worst[1], ey)]
    return worst


def _table(mode, ks, **params):
    """_compare over the three batches and `ks`; prints the worst ratios per k and returns the
    largest."""
    top = 0.0
    for k in ks:
        row = {}
        for name in admm_ref.batches():
            row[name] = _compare(name, mode, k, **params)
        print(mode, params, "k", k, {n: "u %.3g y %.3g" % tuple(v) for n, v in row.items()})
        top = max([top] + [x for v in row.values() for x in v])
    return top


@pytest.mark.parametrize("mode", list(MODES))
def test_iterates_default(mode):
    """z_k and y_k at the defaults, adaptation off, k = 1, 2, 3, 5, 8, 30."""
    assert _table(mode, admm_ref.KS, adaptive_rho_interval=0) <= 1.0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("params", admm_ref.OFF_DEFAULT, ids=_ids(admm_ref.OFF_DEFAULT))
def test_iterates_off_default(params, mode):
    """One of alpha, rho, sigma off its default: the kernel must use the plan's value."""
    assert _table(mode, admm_ref.KS_OFF, adaptive_rho_interval=0, **params) <= 1.0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("interval,max_iter", admm_ref.ADAPT_RUNS)
def test_rho_adaptation(interval, max_iter, mode):
    """rho adapts every second or third iteration from admm_ref.ADAPT (where the reference's
    decisions are clear): the period wraps, and at (2, 8) and (3, 9) the last iteration is one at
    which rho would adapt (it must not).  Compared on the instances whose every decision the
    reference takes with a margin (tests/test_admm_ref.py asserts that they are >= 75 %)."""
    params = dict(adaptive_rho_interval=interval, **admm_ref.ADAPT)
    top = 0.0
    for name in admm_ref.batches():
        refs = admm_ref.reference(name, max_iter, **params)
        only = [r is not None and admm_ref.clear_rho(r) for r in refs]
        w = _compare(name, mode, max_iter, only=only, **params)
        print(mode, params, "k", max_iter, name, "u %.3g y %.3g" % tuple(w))
        top = max(top, *w)
    assert top <= 1.0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("rel", [False, True], ids=["eps_abs", "eps_rel"])
@pytest.mark.parametrize("run", admm_ref.STATUS_RUNS, ids=_ids(admm_ref.STATUS_RUNS))
def test_exit_status(run, rel, mode):
    """Status 2 or -2 at max_iter from the last iteration's residuals (in the second run the
    values stored at the adaptation iteration 25 must have been overwritten): with the tolerance
    4 x the largest reference residual every instance returns 2, with 1 / 4 of the smallest -2,
    and with the middle one (admm_ref.status_eps) the reference's verdict on the instances where
    it is clear.  eps_abs alone tests rp and rd, eps_rel alone their scales np and nd."""
    name = admm_ref.STATUS_BATCH
    refs = admm_ref.reference(name, **run)
    hi, lo, mid, clear, verdict = admm_ref.status_eps(refs, rel)
    got = {}
    for tag, eps in (("hi", hi), ("lo", lo), ("mid", mid)):
        kw = dict(eps_abs=0.0, eps_rel=eps) if rel else dict(eps_abs=eps, eps_rel=0.0)
        got[tag] = _solve(name, mode, **run, **kw)[2]
        print(mode, run, tag, "%.3g" % eps, got[tag].tolist())
    print("reference", verdict.tolist(), "clear", clear.astype(int).tolist())
    assert np.all(got["hi"] == 2), got["hi"]
    assert np.all(got["lo"] == -2), got["lo"]
    assert np.all(got["mid"][clear] == verdict[clear]), np.flatnonzero(got["mid"] != verdict)


@pytest.mark.parametrize("mode", list(MODES))
def test_lam_out_unpolished(mode):
    """lam_out at an unpolished exit against include/cmpc.h's formulas in float64 at the device's
    own u (admm_ref.multipliers); legs between 1e-7 and 1e-4 relative of a face are ambiguous
    (the kernel draws the line at 1e-5) and left out, at most 5 % of the stance legs."""
    top = 0.0
    for k in (1, 8, 30):
        for name, (N, b) in admm_ref.batches().items():
            U, X, st, it, lam = _solve(name, mode, k, want="lam", adaptive_rho_interval=0)
            namb = 0
            for i, p in enumerate(admm_ref.batch_problems(name)):
                ref, amb = admm_ref.multipliers(p, admm_ref.instance(b, i), U[i])
                namb += int(amb.sum())
                keep = admm_ref.lam_compared(amb)
                scale = admm_ref.BAR_FACTOR * admm_ref.LAM_D * float(np.max(np.abs(ref)))
                e = float(np.max(np.abs(lam[i] - ref)[keep])) / scale
                if e > 1:
                    print(f"  over the bar: {name}[{i}] n={p.n} k={k} lam {e:.3g}")
                top = max(top, e)
            assert namb <= 0.05 * sum(p.n // 3 for p in admm_ref.batch_problems(name)), (name, namb)
        print(mode, "k", k, "lam worst ratio so far %.3g" % top)
    assert top <= 1.0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("knob", KNOBS, ids=_ids(KNOBS))
def test_knobs_polished(knob, mode):
    """One knob off its default with the polish on: the certified optima at the bars of
    test_gpu_admm_passes._check (tests/test_admm_ref.py: the model alone returns status 1 on all
    16 instances for every set).  The trigger's arithmetic: from a cold start the face set can
    have been unchanged for polish_stable = s iterations at iteration s + 1 at the earliest, and
    with s = 1 some instance is polished at iteration 2 (the model: two of them)."""
    import torch
    from cmpc import Plan, SolverParams, solve_batch
    b = batch(16)
    plan = Plan(SolverParams(max_batch=64, **knob))
    plan.set_team(MODES[mode])
    w, st, it = solve_batch(b, plan=plan)
    plan.close()
    print(mode, knob, "iters", it.tolist())
    _check(b, w, st, load_fixture("qp_admm_passes.npz")["w16"], 16)
    s = knob.get("polish_stable", 3)
    assert np.all(it >= s + 1), it
    if s == 1:
        assert np.any(it == 2), it


@pytest.mark.parametrize("field", ["eps_abs", "eps_rel"])
@pytest.mark.parametrize("value", [-1e-4, float("nan"), float("inf")])
def test_eps_validated(field, value):
    from cmpc import Plan, SolverParams
    from cmpc.solver import CmpcError
    with pytest.raises(CmpcError, match="eps_abs and eps_rel"):
        Plan(SolverParams(max_batch=64, **{field: value}))
    Plan(SolverParams(max_batch=64, **{field: 0.0})).close()
