"""Shared by tests/test_srb_fb.py (CPU) and tests/test_gpu_srb_fb.py (TEST INFRASTRUCTURE): a
float64 / float32 oracle of the plant step with the first-order force law and an external wrench
(``cmpc_srb_step_io_run``, include/cmpc.h), its input generator and the tolerance
rule.

The oracle is ``oracle.srb_ref.srb_step``'s loop, restated from the same pieces
(``srb_ref.Plant``, ``srb_ref.stance_mask``) with the forces recomputed at every substep; with
every option off it performs the same operations in the same order and equals it bit for bit.
``dtype=np.float32`` rounds every state operation, the difference x_s - x_solve, the rounded
forces and the clamps to float32; ``K``, the row sums, the time and the gait phase stay float64,
as in the kernel.  :class:`Law` holds one overridable piece per decision of the law, for the
deliberate mistakes of tests/test_srb_fb.py."""
from __future__ import annotations

import numpy as np

from oracle import srb_ref
from srb_util import EPS32, GROUPS, f32, group_diff, group_scale, make_plant_inputs

N_PLAN = 16                        # the default plan's horizon: contact is (B, 4, N_PLAN)
MU0, FZ0 = 0.8, 10.0               # the default plan's constants (cmpc_params_default)
R_BLOCK = 64                       # robots per block of srb_feedback_kernel (kSrbFbRobots)
FB_GROUPS = GROUPS + ("force",)
MPC_DT = 1.0 / 3 / 16
K_ROT = 0.1 / 0.2                  # roll inertia over a hip lever (kg m): the 'mass' a force sees in rotation
OPTIONS = ("K", "x_solve", "contact", "mu", "fz_min", "wrench")

# (B, seed) of the draws the GPU test steps on the device: the block edge on both sides, one
# robot, two blocks and one robot
FB_CASES = [(1, 1101), (R_BLOCK - 1, 1163), (R_BLOCK, 1164), (R_BLOCK + 1, 1165),
            (2 * R_BLOCK + 1, 1229)]


class Law:
    """The documented force law and wrench, one overridable piece per decision."""

    @staticmethod
    def delta(x_s, x_solve, x_tick):
        """What the gain multiplies: the substep's state minus the solve's."""
        return x_s - x_solve

    @staticmethod
    def gain(K):
        return K

    @staticmethod
    def clamp(u, mu, fz_min):
        """(B,4,3) forces into the friction pyramid: fz first, the tangential bounds from it."""
        fz = np.maximum(u[:, :, 2], fz_min[:, None])
        lim = mu[:, None] * fz
        return np.stack([np.minimum(np.maximum(u[:, :, 0], -lim), lim),
                         np.minimum(np.maximum(u[:, :, 1], -lim), lim), fz], 2)

    @staticmethod
    def legs(plan_stance):
        """(B,4) bool: the legs that receive feedback and clamp."""
        return plan_stance

    @staticmethod
    def wrench(wr, R, stance):
        """(force, torque) added to F and T."""
        return wr[:, 0:3], wr[:, 3:6]


def valid_terrain(mu, fz_min):
    """cmpc_solve_io's rule for a (mu, fz_min) entry."""
    return np.isfinite(mu) & (mu > 0) & np.isfinite(fz_min)


def fb_step(inp, h, nsub, dtype=np.float64, model=srb_ref.Plant, law=Law, use=OPTIONS):
    """``nsub`` substeps of length ``h``.  ``inp``: make_plant_inputs' keys plus the options
    ``use`` names (a missing or unnamed option is off: NULL).  Returns a dict: x, feet, contact
    (the three of srb_step), force_out (B,12), fb_status (B,) uint8 and margin (B,), the smallest
    distance of a pre-clamp force component of a leg that applied its force from the clamp
    boundary it is compared with (inf for a robot without the law)."""
    ft = np.dtype(dtype).type
    opt = {k: inp.get(k) if k in use else None for k in OPTIONS}
    x = np.array(inp["x"], dtype=ft)
    B = x.shape[0]
    p, rpy, v, w = x[:, 0:3].copy(), x[:, 3:6].copy(), x[:, 6:9].copy(), x[:, 9:12].copy()
    feet = np.array(inp["feet"], dtype=ft).reshape(B, 4, 3)
    f0 = np.asarray(inp["force"], dtype=ft).reshape(B, 4, 3)
    m = np.asarray(inp["mass"], dtype=ft).reshape(B)
    Ib = np.asarray(inp["inertia_body"], dtype=ft).reshape(B, 3, 3)
    hip = np.asarray(inp["hip"], dtype=ft).reshape(4, 3)
    gait = np.asarray(inp["gait"], np.float64)
    period, duty, offs = gait[:, 0], gait[:, 1], gait[:, 2:6]
    t_stance = (duty * period).astype(ft)
    t = np.array(inp["t_now"], np.float64).reshape(B)
    hs = ft(h)
    g = np.array([0, 0, -srb_ref.GRAVITY], dtype=ft)
    bits = np.asarray(inp["contact_state"], np.uint8).reshape(B)
    stance = ((bits[:, None] >> np.arange(4, dtype=np.uint8)) & 1).astype(bool)
    has_law = np.zeros(B, bool)
    if opt["K"] is not None:
        K = np.asarray(opt["K"], np.float64).reshape(B, 12, 12)
        mu = np.full(B, MU0) if opt["mu"] is None else np.asarray(opt["mu"], np.float64)
        fzm = np.full(B, FZ0) if opt["fz_min"] is None else np.asarray(opt["fz_min"], np.float64)
        has_law = np.isfinite(K).all((1, 2)) & valid_terrain(mu, fzm)
        Kl = np.where(has_law[:, None, None], law.gain(K), 0.0)
        mu, fzm = mu.astype(ft), fzm.astype(ft)
        xs = np.asarray(opt["x_solve"], dtype=ft).reshape(B, 12)
        plan_stance = np.asarray(opt["contact"]).reshape(B, 4, -1)[:, :, 0] != 0
        fb_legs = law.legs(plan_stance) & has_law[:, None]
    wr = None if opt["wrench"] is None else np.asarray(opt["wrench"], dtype=ft).reshape(B, 6)
    clamped = np.zeros(B, bool)
    margin = np.full(B, np.inf)
    f = f0
    for _ in range(int(nsub)):
        now = srb_ref.stance_mask(model.contact_time(t, float(h)), period, duty, offs)
        for leg in range(4):
            land = now[:, leg] & ~stance[:, leg]
            if land.any():
                td = model.touchdown(p, rpy[:, 2], v, hip[leg], t_stance)
                feet[land, leg] = td[land]
        stance = now
        if opt["K"] is not None:
            d = law.delta(np.concatenate([p, rpy, v, w], 1), xs, x).astype(np.float64)
            u = (f0.reshape(B, 12).astype(np.float64)
                 + np.einsum('bij,bj->bi', Kl, d)).astype(ft).reshape(B, 4, 3)
            with np.errstate(invalid="ignore"):
                c = law.clamp(u, mu, fzm)
            f = np.where(fb_legs[:, :, None], c, f0)
            acts = fb_legs & stance
            clamped |= np.any(acts & np.any(c != u, 2), 1)
            lim = mu[:, None].astype(np.float64) * np.asarray(c[:, :, 2], np.float64)
            u64 = u.astype(np.float64)
            dist = np.minimum(np.abs(u64[:, :, 2] - fzm[:, None]),
                              np.minimum(np.abs(np.abs(u64[:, :, 0]) - lim),
                                         np.abs(np.abs(u64[:, :, 1]) - lim)))
            margin = np.minimum(margin, np.where(acts, dist, np.inf).min(1))
        R = model.rotation(rpy)
        Iw = model.inertia_world(R, Ib)
        fs = f * stance[:, :, None].astype(ft)
        lever = feet - p[:, None, :]
        torque = np.cross(lever, fs).sum(1)
        total = fs.sum(1)
        if wr is not None:
            wf, wt = law.wrench(wr, R, stance)
            total, torque = total + wf, torque + wt
        v_new = v + hs * (total / m[:, None] + g)
        wd = np.linalg.solve(Iw, (torque - model.gyroscopic(w, Iw))[:, :, None])[:, :, 0]
        w = w + hs * wd
        p = model.advance_position(p, v, v_new, hs)
        v = v_new
        rpy = rpy + hs * model.euler_rates(rpy, w)
        t = t + float(h)
    out = (stance.astype(np.uint8) << np.arange(4, dtype=np.uint8)).sum(1).astype(np.uint8)
    status = np.where(has_law, np.where(clamped, 2, 1), 0).astype(np.uint8)
    return dict(x=np.concatenate([p, rpy, v, w], 1), feet=feet, contact=out,
                force_out=np.array(f).reshape(B, 12), fb_status=status, margin=margin)


def make_fb_inputs(B: int, seed: int, h: float = None) -> dict:
    """make_plant_inputs' robots with the options of the extended step.

    ``K``: no fixture holds gains, so entries are log-uniform over three decades with random
    signs, up to m / dt^2 in the position columns and m / dt in the velocity columns (m = 15 kg,
    dt the MPC step), and up to their rotational analogues (I / lever) / dt^2 and (I / lever) / dt
    in the angle and angular-velocity columns (K_ROT).  A gain of the MPC is stabilising; one with
    random signs is not, and at m / dt^2 = 34,560 N / rad the attitude loop (lever x force / I)
    has a growth rate of 260 / s and a rate gain of m / dt = 720 N s / rad multiplies w by 2.4 per
    substep: the float32 oracle then leaves the float64 one by many orders of magnitude within
    twenty substeps (or overflows) and no tolerance derived from it says anything.  ``x_solve`` = x + offsets of up to 2e-3; the step-0 column of
    ``contact`` is stance with probability 3/4 and the other columns are random; mu ~ U(0.2, 1),
    fz_min ~ U(0, 20); wrenches up to 100 N and 20 N m.  Four robots in ten are 'gentle':
    forces well inside their pyramid and a gain a few thousand times smaller, so that the law
    is applied without a clamp (fb_status 1).  Another 48 % are 'steady': the same small gain
    around the generator's forces with fz ~ U(0, 40), many of which lie outside the pyramid, so
    that the same clamps hold over the whole call.  The remaining 12 % carry the full gain:
    its forces sweep across the clamp boundaries, and those are the robots that can end within
    the force tolerance of one (tests/test_srb_fb.py bounds their share).  About one robot in twenty has a NaN or Inf in K
    and one in twenty an invalid mu or fz_min; robot 0 never, so a batch of one has the law."""
    inp = make_plant_inputs(B, seed) if h is None else make_plant_inputs(B, seed, h)
    rng = np.random.default_rng(seed + 7919)
    top = np.repeat([15.0 / MPC_DT ** 2, K_ROT / MPC_DT ** 2, 15.0 / MPC_DT, K_ROT / MPC_DT], 3)
    K = top * 10.0 ** rng.uniform(-3, 0, (B, 12, 12)) * rng.choice([-1.0, 1.0], (B, 12, 12))
    mu = f32(rng.uniform(0.2, 1.0, B))
    fz_min = f32(rng.uniform(0.0, 20.0, B))
    kind = rng.random(B)
    gentle, steady = kind < 0.4, (kind >= 0.4) & (kind < 0.88)
    K[gentle | steady] *= 3e-4
    force = inp["force"].reshape(B, 4, 3).copy()
    force[steady, :, 2] = rng.uniform(0, 40, (B, 4))[steady]
    fz = fz_min[:, None] + rng.uniform(10, 60, (B, 4))
    tang = rng.uniform(-0.3, 0.3, (B, 4, 2)) * (mu[:, None] * fz)[:, :, None]
    force[gentle, :, 2] = fz[gentle]
    force[gentle, :, 0:2] = tang[gentle]
    inp["force"] = f32(force.reshape(B, 12))
    bad_k = (rng.random(B) < 0.05) & (np.arange(B) > 0)
    for b in np.flatnonzero(bad_k):
        K[b, rng.integers(12), rng.integers(12)] = rng.choice([np.nan, np.inf, -np.inf])
    bad_mu = (rng.random(B) < 0.05) & (np.arange(B) > 0)
    for b in np.flatnonzero(bad_mu):
        if rng.random() < 0.75:
            mu[b] = rng.choice([0.0, -0.5, np.nan, np.inf])
        else:
            fz_min[b] = rng.choice([np.nan, np.inf])
    contact = (rng.random((B, 4, N_PLAN)) < 0.5).astype(np.uint8)
    contact[:, :, 0] = rng.random((B, 4)) < 0.75
    wrench = np.concatenate([rng.uniform(-100, 100, (B, 3)), rng.uniform(-20, 20, (B, 3))], 1)
    inp.update(K=K, x_solve=f32(inp["x"] + rng.uniform(-2e-3, 2e-3, (B, 12))), contact=contact,
               mu=mu, fz_min=fz_min, wrench=f32(wrench), gentle=gentle, bad_k=bad_k,
               bad_mu=bad_mu)
    return inp


def as_triple(r):
    return r["x"], r["feet"], r["contact"]


def fb_diff(a, b):
    """max |a - b| per group of two fb_step results: srb_util's five and the forces."""
    d = group_diff(as_triple(a), as_triple(b))
    d["force"] = float(np.abs(np.asarray(a["force_out"], np.float64)
                              - np.asarray(b["force_out"], np.float64)).max(initial=0.0))
    return d


def fb_scale(r):
    d = group_scale(as_triple(r))
    d["force"] = float(np.abs(np.asarray(r["force_out"], np.float64)).max(initial=0.0))
    return d


def fb_yardstick(inp, h, nsub, use=OPTIONS):
    """(oracle64, oracle32, d_g = max |oracle32 - oracle64| per group) of the extended step."""
    r64 = fb_step(inp, h, nsub, use=use)
    r32 = fb_step(inp, h, nsub, dtype=np.float32, use=use)
    return r64, r32, fb_diff(r32, r64)


def fb_tolerances(r64, d):
    """srb_util's rule with force_out as a sixth group: 8 d_g + 4 * 2^-24 * max |oracle64_g|."""
    sc = fb_scale(r64)
    return {g: 8.0 * d[g] + 4.0 * EPS32 * sc[g] for g in FB_GROUPS}


def status_comparable(r64, tol_force):
    """The robots whose fb_status the device must reproduce: every pre-clamp force of a leg that
    applied it is further from its clamp boundary than the force tolerance."""
    return r64["margin"] > tol_force


def check_fb_against_oracle(got, inp, h, nsub, use=OPTIONS, label=""):
    """``got``: dict of the device's x, feet, contact, force_out, fb_status.  Contact bits exact,
    every group within the tolerance, fb_status exact where comparable.  Prints and returns the
    per-group ratio (device error) / (float32 yardstick)."""
    r64, r32, d = fb_yardstick(inp, h, nsub, use)
    np.testing.assert_array_equal(r32["contact"], r64["contact"])
    np.testing.assert_array_equal(np.asarray(got["contact"]), r64["contact"])
    err, tol = fb_diff(got, r64), fb_tolerances(r64, d)
    ratio = {g: (err[g] / d[g] if d[g] > 0 else 0.0) for g in FB_GROUPS}
    ok = status_comparable(r64, tol["force"])
    print(f"{label} status compared on {int(ok.sum())}/{len(ok)}; device error / float32 "
          "yardstick: " + ", ".join(f"{g} {ratio[g]:.2f} ({err[g]:.2e} / {d[g]:.2e})"
                                    for g in FB_GROUPS))
    for g in FB_GROUPS:
        assert err[g] <= tol[g], (label, g, err[g], tol[g], d[g])
    np.testing.assert_array_equal(np.asarray(got["fb_status"])[ok], r64["fb_status"][ok])
    return ratio
