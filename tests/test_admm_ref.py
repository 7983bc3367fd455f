"""The float64 ADMM reference (tests/admm_ref.py) is right, and the bar of the GPU tests
(tests/test_gpu_admm_iterates.py) is set: all on the CPU.

(a) Convergence: 3,000 iterations with the rho adaptation on reach the certified optimum of
    tests/golden/qp_admm_passes.npz within 1e-6 x max(1, max|u|) on every instance of
    test_gpu_admm_passes.batch(16) (measured: <= 3.0e-7), so the reference iterates the right QP.
(b) Agreement with the model: with the adaptation off, z_k against tests/algo_spec.py's U at
    max_iter = k (an independent fp32 implementation), worst deviation over the batch relative to
    S = max(1, max|z_ref|), measured here:

        k                      1        2        3        5        8        30
        exact factor           9.8e-5   2.6e-5   3.0e-5   1.3e-5   4.5e-6   7.1e-7
        fp32_admm=True  (D_k)  1.83e-4  7.43e-5  8.38e-5  3.13e-5  7.60e-6  8.90e-7
        admm_ref.D_K           2.0e-4   8.2e-5   9.2e-5   3.5e-5   8.4e-6   1.0e-6

    admm_ref.D_K is the fp32 row with 10 % headroom (the model's matrix-vector products go
    through the BLAS, whose summation order may differ between machines); the GPU bar at k is
    4 x D_K[k].  The factor 4 covers the kernel's LDL' factor and summation order against the
    model's sweep inverse, and the team and wave modes ordering their sums differently.
(c) Sensitivity: alpha 1.6 -> 1.5, rho 1e-4 -> 1.2e-4 and sigma 1e-6 -> 1e-5, one at a time, move
    the reference's z_k at k = 1, 2, 3 by at least 10 x (4 D_K[k]) on every instance (measured
    smallest shifts: alpha 6.2e-2 / 4.3e-2 / 2.3e-2, rho 1.7e-2 / 1.6e-2 / 1.2e-2, sigma 1.1e-2 /
    1.1e-2 / 1.1e-2, against 10 x 4 D_K = 8.0e-3 / 3.3e-3 / 3.7e-3).  The bar may never be raised
    past this.
    alpha = 1.9 and rho = 1e-5 have tables of their own (admm_ref.D_OFF, measured the same way
    over the 22 instances of admm_ref.batches()["main"]: 2.74e-4 / 3.37e-4 / 4.57e-4 and 5.94e-4 /
    4.31e-4 / 5.1e-5 at k = 1, 3, 8); there the default value in place of the plan's moves z_k by
    at least 10 x the bar on every instance (smallest shifts 0.158 / 0.105 / 0.035 and 0.127 /
    0.069 / 0.0056).
(d) Clear decisions: the instances the GPU's adaptive and status runs compare are those whose
    decisions the reference takes with a margin (admm_ref.clear_rho, clear_status); at most 25 %
    of a run's instances may be left out.  At the default rho and alpha the cap cannot be met at
    intervals 2 and 3: rho' / rho falls through the 1 / 5 threshold smoothly as rp shrinks, so
    16 .. 22 of the 30 instances decide within 25 % of it.  The adaptive runs therefore start
    from alpha = 1.4, rho = 0.05 (admm_ref.ADAPT): 3, 3, 0, 0 of 30 left out at (interval,
    max_iter) = (2, 8), (2, 9), (3, 8), (3, 9), every instance changes rho (twice at (2, 9)),
    and a run that did not adapt misses the bar by a factor >= 18.  The status runs use `main`
    (2 of 22 left out, for their rho decision at iteration 25) with the middle tolerance of
    admm_ref.status_eps.
(e) The off-default knob sets of the GPU file's polished runs are solved (status 1 on all 16
    instances) by the model alone, so "at most one status 2 per batch" is reachable.
(f) The lam_out bar: the float32 evaluation of include/cmpc.h's multiplier formulas against the
    float64 one at the reference's z_k.
"""
import numpy as np
import pytest

import admm_ref
import algo_spec
from parity_util import load_fixture, split_w

KS_MODEL = (1, 2, 3, 5, 8, 30)
PERTURB = (dict(alpha=1.5), dict(rho=1.2e-4), dict(sigma=1e-5))
# the off-default sets of test_gpu_admm_iterates.py::test_knobs_polished in the model's names
KNOBS = ([dict(alpha=v) for v in (1.0, 1.9)] + [dict(rho=v) for v in (1e-5, 1e-3)] +
         [dict(sigma=v) for v in (0.0, 1e-4)] + [dict(stable_checks=v) for v in (1, 6)] +
         [dict(repairs=v) for v in (0, 1)] + [dict(adaptive_interval=0)])


@pytest.fixture(scope="module")
def b16():
    from test_gpu_admm_passes import batch
    b = batch(16)
    return b, admm_ref.problems(b)


def _S(v):
    return max(1.0, float(np.max(np.abs(v))))


def test_converges_to_certified_optimum(b16):
    b, probs = b16
    _, Ur = split_w(load_fixture("qp_admm_passes.npz")["w16"].astype(np.float64))
    worst = 0.0
    for i, p in enumerate(probs):
        r = admm_ref.run(p, 3000)
        err = np.max(np.abs(p.full(r["z"][-1]) - Ur[i].reshape(-1))) / _S(Ur[i])
        worst = max(worst, err)
        assert err <= 1e-6, (i, err)
    print("worst", worst)


def test_agrees_with_model_and_sets_bar(b16):
    b, probs = b16
    refs = [admm_ref.run(p, max(KS_MODEL), adaptive_rho_interval=0) for p in probs]
    D = {fp: {} for fp in (False, True)}
    for fp in (False, True):
        for k in KS_MODEL:
            d = 0.0
            for i, p in enumerate(probs):
                m = algo_spec.solve(admm_ref.instance(b, i), algo_spec.Params(
                    max_iter=k, stable_checks=10**6, adaptive_interval=0, fp32_admm=fp))
                assert m["iters"] == k and m["status"] == -2
                zr = p.full(refs[i]["z"][k - 1])
                d = max(d, float(np.max(np.abs(m["U"].reshape(-1) - zr))) / _S(zr))
            D[fp][k] = d
        print("fp32_admm", fp, {k: "%.3g" % v for k, v in D[fp].items()})
    for k in KS_MODEL:
        # the table is the fp32 column with its headroom, and is not looser than that
        assert D[True][k] <= admm_ref.D_K[k], (k, D[True][k])
        assert D[True][k] >= 0.7 * admm_ref.D_K[k], (k, D[True][k])
        assert D[False][k] <= admm_ref.D_K[k], (k, D[False][k])
    assert set(admm_ref.KS) <= set(admm_ref.D_K)


def test_bar_catches_a_wrong_parameter(b16):
    b, probs = b16
    for kw in PERTURB:
        for k in (1, 2, 3):
            shifts = []
            for p in probs:
                z0 = admm_ref.run(p, k, adaptive_rho_interval=0)["z"][-1]
                z1 = admm_ref.run(p, k, adaptive_rho_interval=0, **kw)["z"][-1]
                shifts.append(float(np.max(np.abs(z1 - z0))) / _S(z0))
            print(kw, k, "smallest shift %.3g" % min(shifts), "bar %.3g" % admm_ref.bar(k))
            assert min(shifts) >= 10 * admm_ref.bar(k), (kw, k, min(shifts))


def test_off_default_bars():
    """The two off-default values with a table of their own (admm_ref.D_OFF): the table is the
    fp32 model's deviation over the `main` batch, and a kernel that used the default instead of
    the plan's value would miss the bar by a factor >= 10 at every k on every instance."""
    N, b = admm_ref.batches()["main"]
    probs = admm_ref.batch_problems("main")
    for (key, val), table in admm_ref.D_OFF.items():
        for k in admm_ref.KS_OFF:
            refs = admm_ref.reference("main", k, adaptive_rho_interval=0, **{key: val})
            dflt = admm_ref.reference("main", k, adaptive_rho_interval=0)
            d, shifts = 0.0, []
            for i, p in enumerate(probs):
                m = algo_spec.solve(admm_ref.instance(b, i), algo_spec.Params(
                    max_iter=k, stable_checks=10**6, adaptive_interval=0, fp32_admm=True,
                    **{key: val}))
                zr = refs[i]["z"][-1]
                d = max(d, float(np.max(np.abs(m["U"].reshape(-1) - p.full(zr)))) / _S(zr))
                shifts.append(float(np.max(np.abs(dflt[i]["z"][-1] - zr))) / _S(zr))
            print(key, val, k, "D %.3g" % d, "smallest shift from the default %.3g" % min(shifts))
            assert 0.7 * table[k] <= d <= table[k], (key, k, d)
            assert min(shifts) >= 10 * admm_ref.bar(k, **{key: val}), (key, k, min(shifts))


def _share(flags):
    return 1.0 - sum(flags) / len(flags)


def test_clear_decisions_cap():
    """Every adaptive and status run of the GPU file leaves at most 25 % of its instances out;
    the adaptive runs change rho on every instance, twice where the period allows it."""
    names = list(admm_ref.batches())
    for iv, mi in admm_ref.ADAPT_RUNS:
        rs = [r for nm in names for r in admm_ref.reference(
            nm, mi, adaptive_rho_interval=iv, **admm_ref.ADAPT) if r is not None]
        clear = [admm_ref.clear_rho(r) for r in rs]
        changes = [len(np.unique(r["rho"])) - 1 for r in rs]
        print("adapt", iv, mi, "left out", [i for i, c in enumerate(clear) if not c],
              "rho changes", changes)
        assert _share(clear) <= admm_ref.MAX_EXCLUDED
        assert min(changes) >= 1
        # the bar after the last change of rho catches a run that did not adapt
        fixed = [r for nm in names for r in admm_ref.reference(
            nm, mi, adaptive_rho_interval=0, **admm_ref.ADAPT) if r is not None]
        shift = [float(np.max(np.abs(r["z"][-1] - f["z"][-1]))) / _S(r["z"][-1]) /
                 admm_ref.bar(admm_ref.since_refactor(r)) for r, f, c in zip(rs, fixed, clear) if c]
        print("  smallest shift without adaptation / bar %.3g" % min(shift))
        assert min(shift) >= 10
    for run in admm_ref.STATUS_RUNS:
        rs = admm_ref.reference(admm_ref.STATUS_BATCH, **run)
        for rel in (False, True):
            hi, lo, mid, clear, verdict = admm_ref.status_eps(rs, rel)
            eps = dict(eps_abs=0.0, eps_rel=mid) if rel else dict(eps_abs=mid, eps_rel=0.0)
            rm = admm_ref.reference(admm_ref.STATUS_BATCH, **run, **eps)
            print("status", run, "rel" if rel else "abs", "eps", (hi, lo, mid), "left out",
                  np.flatnonzero(~clear).tolist(), "verdicts", verdict.tolist())
            assert [r["status"] for r in rm] == verdict.tolist()
            assert all(admm_ref.clear_status(r) for r, c in zip(rm, clear) if c)
            assert _share(clear) <= admm_ref.MAX_EXCLUDED
            assert set(verdict[clear].tolist()) == {2, -2}   # both verdicts occur


def test_model_solves_the_knob_sets(b16):
    b, _ = b16
    for kw in KNOBS:
        res = [algo_spec.solve(admm_ref.instance(b, i), algo_spec.Params(
            fp32_polish=True, downdate=True, dd_max=6, polish_refine=2, **kw))
            for i in range(len(b["Ad"]))]
        it = [r["iters"] for r in res]
        print(kw, "iters", min(it), max(it))
        assert all(r["status"] == 1 for r in res), (kw, [r["status"] for r in res])
        if kw == dict(stable_checks=1):
            assert sum(i == 2 for i in it) >= 1, it


def test_lam_bar(b16):
    b, probs = b16
    worst = 0.0
    for k in (1, 8, 30):
        for i, p in enumerate(probs):
            inst = admm_ref.instance(b, i)
            u = p.full(admm_ref.run(p, k, adaptive_rho_interval=0)["z"][-1]).astype(np.float32)
            l64, amb = admm_ref.multipliers(p, inst, u)
            l32, _ = admm_ref.multipliers(p, inst, u, dtype=np.float32)
            assert amb.sum() <= 0.05 * (np.asarray(inst["contact"]) != 0).sum(), (k, i, amb.sum())
            keep = admm_ref.lam_compared(amb)
            worst = max(worst, float(np.max(np.abs(l32 - l64)[keep]) / np.max(np.abs(l64))))
    print("worst fp32 deviation of lam %.3g" % worst)
    assert worst <= admm_ref.LAM_D and worst >= 0.5 * admm_ref.LAM_D
