"""CPU: the oracle of the plant step with the force law and a wrench (tests/srb_fb_util.py) and
the inputs the GPU test (tests/test_gpu_srb_fb.py) steps on the device.

Part 1: with every option off the oracle is ``srb_ref.srb_step`` bit for bit, and the wrench
obeys the momentum balance it was not built from.  Part 2: conditions on the GPU test's inputs --
every clamp outcome and every fb_status value occurs often, few robots sit so close to a clamp
boundary that float32 rounding could decide their status, and no contact bit hangs on rounding.
Part 3: eight deliberate mistakes in the law or the wrench each move some state group by at
least 100 float32 yardsticks on those inputs; the GPU test allows the kernel 8."""
import numpy as np
import pytest

from oracle import srb_ref
from srb_fb_util import (FB_CASES, FB_GROUPS, OPTIONS, R_BLOCK, Law, fb_diff, fb_step,
                         fb_tolerances, fb_yardstick, make_fb_inputs, status_comparable)
from srb_util import GROUPS, H, bits_mask, make_plant_inputs, oracle, phase_margin

B_BIG, SEED_BIG = FB_CASES[-1]


# ---------------------------------------------------------------- 1. the oracle itself

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nsub", [1, 20])
def test_options_off_is_srb_step(nsub, dtype):
    inp = make_fb_inputs(B_BIG, SEED_BIG)
    got = fb_step(inp, H, nsub, dtype=dtype, use=())
    x, feet, contact = oracle(inp, H, nsub, dtype=dtype)
    assert got["x"].dtype == x.dtype
    assert np.array_equal(got["x"], x) and np.array_equal(got["feet"], feet)
    assert np.array_equal(got["contact"], contact)
    assert np.array_equal(got["force_out"], np.asarray(inp["force"], dtype))
    assert np.all(got["fb_status"] == 0) and np.all(np.isinf(got["margin"]))


def _free_flight(Bn=8, seed=3):
    """Robots whose four legs stay in swing for as long as the tests integrate."""
    inp = make_fb_inputs(Bn, seed)
    inp["gait"][:, 0] = 0.5
    inp["gait"][:, 1] = 0.4
    inp["gait"][:, 2:6] = 0.45
    inp["t_now"][:] = 0.0
    inp["contact_state"][:] = 0
    return inp


def test_free_flight_momentum_under_a_wrench():
    """All legs in swing: m v changes by (wrench force + m g) nsub h and nothing else, the law's
    forces never being applied."""
    inp = _free_flight()
    nsub, h = 20, 1e-3
    r = fb_step(inp, h, nsub)
    assert np.all(r["contact"] == 0)
    m = inp["mass"][:, None]
    dP = m * (r["x"][:, 6:9] - inp["x"][:, 6:9])
    want = (inp["wrench"][:, 0:3] + m * np.array([0, 0, -srb_ref.GRAVITY])) * nsub * h
    assert np.abs(dP - want).max() < 1e-12 * np.abs(want).max()


def test_pure_torque_moves_only_the_attitude():
    inp = _free_flight()
    inp["wrench"][:, 0:3] = 0.0
    with_t = fb_step(inp, 1e-3, 20, use=("wrench",))
    without = fb_step(inp, 1e-3, 20, use=())
    assert np.array_equal(with_t["x"][:, 0:3], without["x"][:, 0:3])
    assert np.array_equal(with_t["x"][:, 6:9], without["x"][:, 6:9])
    assert np.array_equal(with_t["feet"], without["feet"])
    assert np.all(np.abs(with_t["x"][:, 9:12] - without["x"][:, 9:12]).max(1) > 1e-3)
    assert np.all(np.abs(with_t["x"][:, 3:6] - without["x"][:, 3:6]).max(1) > 1e-6)


def test_held_robots_hold_U0():
    """NaN-K and invalid-mu robots: status 0, the hold-force state, force_out = U0."""
    inp = make_fb_inputs(B_BIG, SEED_BIG)
    bad = inp["bad_k"] | inp["bad_mu"]
    assert inp["bad_k"].sum() >= 2 and inp["bad_mu"].sum() >= 2
    r = fb_step(inp, H, 20, use=("K", "x_solve", "contact", "mu", "fz_min"))
    hold = fb_step(inp, H, 20, use=())
    assert np.all(r["fb_status"][bad] == 0) and np.all(r["fb_status"][~bad] != 0)
    assert np.array_equal(r["x"][bad], hold["x"][bad]) and np.all(np.isfinite(r["x"]))
    assert np.array_equal(r["force_out"][bad], inp["force"][bad])


# ---------------------------------------------------------------- 2. the GPU test's inputs

def _outcomes(inp, h, nsub):
    """Per applied (robot, leg, substep) triple of the float64 oracle: fz clamped, a tangential
    clamp active, no clamp -- recounted here by re-running the law on the oracle's own states."""
    counts = np.zeros(4)     # triples, fz, tangential, none

    class Counting(Law):
        @staticmethod
        def clamp(u, mu, fz_min):
            c = Law.clamp(u, mu, fz_min)
            Counting.last = (u, c)
            return c
    # fb_step exposes neither the per-substep forces nor the stance, so step one substep at a time
    cur = dict(inp)
    for k in range(nsub):
        r = fb_step(cur, h, 1, law=Counting)
        u, c = Counting.last
        stance = bits_mask(r["contact"])
        plan = np.asarray(inp["contact"])[:, :, 0] != 0
        acts = stance & plan & (r["fb_status"] != 0)[:, None]
        fzc = c[:, :, 2] != u[:, :, 2]
        tc = (c[:, :, 0] != u[:, :, 0]) | (c[:, :, 1] != u[:, :, 1])
        counts += [acts.sum(), (acts & fzc).sum(), (acts & tc).sum(), (acts & ~fzc & ~tc).sum()]
        cur = dict(cur, x=r["x"], feet=r["feet"], contact_state=r["contact"],
                   t_now=cur["t_now"] + h)
    return counts


def test_substep_chaining_matches_one_call():
    """_outcomes' device: twenty calls of one substep are one call of twenty, except that the
    time is then t_now + k h rather than a repeated sum (no contact bit differs on this input)."""
    inp = make_fb_inputs(R_BLOCK + 1, FB_CASES[3][1])
    cur = dict(inp)
    for k in range(3):
        r = fb_step(cur, H, 1)
        cur = dict(cur, x=r["x"], feet=r["feet"], contact_state=r["contact"],
                   t_now=cur["t_now"] + H)
    # x_solve and the tick's start stay the first call's: only Law.delta's third argument differs
    whole = fb_step(inp, H, 3)
    assert np.array_equal(whole["contact"], r["contact"])
    assert np.abs(whole["x"] - r["x"]).max() < 1e-12


def test_coverage_of_the_gpu_inputs():
    counts, status = np.zeros(4), []
    for Bn, seed in FB_CASES:
        inp = make_fb_inputs(Bn, seed)
        counts += _outcomes(inp, H, 20)
        status.append(fb_step(inp, H, 20)["fb_status"])
    status = np.concatenate(status)
    share = counts[1:] / counts[0]
    by_status = [float(np.mean(status == s)) for s in (0, 1, 2)]
    print("applied triples", int(counts[0]), "fz clamped / tangential / none", share,
          "fb_status 0 / 1 / 2", by_status)
    assert counts[0] >= 2000
    assert np.all(share >= 0.10), share
    assert min(by_status) >= 0.05, by_status
    # and on the largest case alone
    big = fb_step(make_fb_inputs(B_BIG, SEED_BIG), H, 20)["fb_status"]
    assert min(np.mean(big == s) for s in (0, 1, 2)) >= 0.05


@pytest.mark.parametrize("use", [OPTIONS, ("K", "x_solve", "contact", "mu", "fz_min")],
                         ids=["all", "K"])
@pytest.mark.parametrize("nsub", [1, 20])
def test_few_robots_sit_on_a_clamp_boundary(nsub, use):
    """fb_status is compared on robots further from every clamp boundary than the force
    tolerance: at most 2 % of the robots of the GPU cases are left out, and the float32 oracle
    agrees with the float64 one on all the others."""
    left, total = 0, 0
    for Bn, seed in FB_CASES:
        inp = make_fb_inputs(Bn, seed)
        r64, r32, d = fb_yardstick(inp, H, nsub, use)
        ok = status_comparable(r64, fb_tolerances(r64, d)["force"])
        assert np.array_equal(r32["fb_status"][ok], r64["fb_status"][ok])
        left, total = left + int((~ok).sum()), total + Bn
    print("left out", left, "of", total)
    assert left <= 0.02 * total


@pytest.mark.parametrize("Bn,seed", FB_CASES)
def test_gpu_inputs_keep_the_phase_margin(Bn, seed):
    inp = make_fb_inputs(Bn, seed)
    assert phase_margin(inp, H, 20) > 1e-9
    base = make_plant_inputs(Bn, seed)
    for k in ("x", "feet", "t_now", "gait", "mass", "inertia_body", "hip", "contact_state"):
        assert np.array_equal(inp[k], base[k]), k
    for k in ("force", "x_solve", "mu", "fz_min", "wrench"):
        a = np.asarray(inp[k])
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64), equal_nan=True), k
    if Bn == 1:
        assert not inp["bad_k"][0] and not inp["bad_mu"][0]


# ---------------------------------------------------------------- 3. discrimination

class DeltaSign(Law):
    @staticmethod
    def delta(x_s, x_solve, x_tick):
        return x_solve - x_s


class GainTransposed(Law):
    @staticmethod
    def gain(K):
        return np.swapaxes(K, 1, 2)


class TangentialFirst(Law):
    """The tangential clamp from the unclamped fz, and only then fz."""
    @staticmethod
    def clamp(u, mu, fz_min):
        lim = mu[:, None] * u[:, :, 2]
        lo, hi = np.minimum(-lim, lim), np.maximum(-lim, lim)
        return np.stack([np.minimum(np.maximum(u[:, :, 0], lo), hi),
                         np.minimum(np.maximum(u[:, :, 1], lo), hi),
                         np.maximum(u[:, :, 2], fz_min[:, None])], 2)


class TangentialUnclampedFz(Law):
    """fz first, but the tangential bounds from the fz before its clamp (a negative fz gives an
    empty interval: the lower bound wins, as min(max(u, -lim), lim) makes it)."""
    @staticmethod
    def clamp(u, mu, fz_min):
        lim = mu[:, None] * u[:, :, 2]
        return np.stack([np.minimum(np.maximum(u[:, :, 0], -lim), lim),
                         np.minimum(np.maximum(u[:, :, 1], -lim), lim),
                         np.maximum(u[:, :, 2], fz_min[:, None])], 2)


class SwingLegsToo(Law):
    @staticmethod
    def legs(plan_stance):
        return np.ones_like(plan_stance)


class DeltaFromTickStart(Law):
    @staticmethod
    def delta(x_s, x_solve, x_tick):
        return x_tick - x_solve


class TorqueInBodyFrame(Law):
    @staticmethod
    def wrench(wr, R, stance):
        return wr[:, 0:3], np.einsum('bij,bj->bi', R, wr[:, 3:6])


class WrenchGatedByContact(Law):
    @staticmethod
    def wrench(wr, R, stance):
        on = stance.any(1)[:, None].astype(wr.dtype)
        return wr[:, 0:3] * on, wr[:, 3:6] * on


# mutation -> the substep counts at which it must show.  The tick's start state is the first
# substep's state, so that mistake is invisible at one substep (asserted below).  The others act
# on the forces or the wrench of every substep and show at once.
MUTATIONS = {
    "delta_sign": (DeltaSign, (1, 20)),
    "gain_transposed": (GainTransposed, (1, 20)),
    "tangential_before_fz": (TangentialFirst, (1, 20)),
    "tangential_with_unclamped_fz": (TangentialUnclampedFz, (1, 20)),
    "feedback_on_swing_legs": (SwingLegsToo, (1, 20)),
    "delta_from_tick_start": (DeltaFromTickStart, (20,)),
    "torque_in_body_frame": (TorqueInBodyFrame, (1, 20)),
    "wrench_gated_by_contact": (WrenchGatedByContact, (1, 20)),
}


@pytest.fixture(scope="module")
def inputs():
    return make_fb_inputs(B_BIG, SEED_BIG)


@pytest.fixture(scope="module")
def baseline(inputs):
    return {n: fb_yardstick(inputs, H, n) for n in (1, 20)}


@pytest.mark.parametrize("nsub", [1, 20])
@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutation_is_visible(inputs, baseline, name, nsub):
    law, when = MUTATIONS[name]
    r64, r32, d = baseline[nsub]
    mut = fb_step(inputs, H, nsub, law=law)
    eff = fb_diff(mut, r64)
    if nsub not in when:
        assert all(eff[g] == 0.0 for g in FB_GROUPS)
        return
    # a mistake that sends a robot to Inf or NaN within the call has moved it by more than any bar
    ratio = {g: (eff[g] / d[g] if np.isfinite(eff[g]) else np.inf) for g in GROUPS if d[g] > 0}
    print(name, "nsub", nsub, {g: f"{r:.0f}x" for g, r in ratio.items()},
          "yardstick", {g: f"{d[g]:.1e}" for g in FB_GROUPS})
    assert max(ratio.values()) >= 100, ratio
