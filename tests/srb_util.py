"""Shared by tests/test_srb.py (CPU) and the GPU tests of the plant (TEST INFRASTRUCTURE):
the input generator, the float32 yardstick and the tolerance rule built on it."""
from __future__ import annotations

import numpy as np

from cmpc import synth
from oracle import srb_ref

H = (1.0 / 3 / 16) / 20            # the closed loop's substep: MPC_DT / 20 (1/960 s)
GROUPS = ("p", "rpy", "v", "w", "feet")
_SLICE = dict(p=slice(0, 3), rpy=slice(3, 6), v=slice(6, 9), w=slice(9, 12))
EPS32 = 2.0 ** -24


def f32(a):
    """Quantise to float32, keep float64 storage (what crosses the ABI as float32)."""
    return np.asarray(a, np.float32).astype(np.float64)


def mask_bits(stance):
    return (stance.astype(np.uint8) << np.arange(4, dtype=np.uint8)).sum(-1).astype(np.uint8)


def bits_mask(bits):
    return ((np.asarray(bits, np.uint8)[:, None] >> np.arange(4, dtype=np.uint8)) & 1).astype(bool)


def make_plant_inputs(B: int, seed: int, h: float = H) -> dict:
    """``B`` robots in general position: tilted, moving, turning, each with its own mass, a full
    (non-diagonal) body inertia and its own gait, at a late time.  ``contact_state`` is the
    stance mask one substep before ``t_now``, so a few legs land or lift at the first substep."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 12))
    x[:, 0:2] = rng.uniform(-1, 1, (B, 2))
    x[:, 2] = synth.Z_DES + rng.uniform(-0.02, 0.02, B)
    x[:, 3:5] = rng.uniform(-0.3, 0.3, (B, 2))
    x[:, 5] = rng.uniform(-np.pi, np.pi, B)
    x[:, 6:9] = rng.uniform(-0.7, 0.7, (B, 3))
    x[:, 9:12] = rng.uniform(-2, 2, (B, 3))
    x = f32(x)
    mass = f32(rng.uniform(10, 20, B))
    S = rng.normal(0, 0.03, (B, 3, 3))
    Ib = f32(synth.INERTIA_BODY[None] + (S + np.swapaxes(S, 1, 2)) / 2)
    hip = f32(synth.HIP_OFFSETS)
    c, s = np.cos(x[:, 5]), np.sin(x[:, 5])
    feet = np.stack([np.stack([x[:, 0] + c * hx - s * hy, x[:, 1] + s * hx + c * hy,
                               np.zeros(B)], -1) for hx, hy in hip[:, :2]], 1)
    feet = f32(feet + rng.uniform(-0.05, 0.05, (B, 4, 3)))
    force = np.empty((B, 4, 3))
    force[:, :, 0:2] = rng.uniform(-20, 20, (B, 4, 2))
    force[:, :, 2] = rng.uniform(10, 80, (B, 4))
    force = f32(force.reshape(B, 12))
    gait = np.concatenate([rng.uniform(0.25, 0.5, (B, 1)), rng.uniform(0.4, 0.8, (B, 1)),
                           rng.uniform(0, 1, (B, 4))], 1)
    t_now = rng.uniform(0, 1000, B)
    contact = mask_bits(srb_ref.stance_mask(t_now - h, gait[:, 0], gait[:, 1], gait[:, 2:6]))
    return dict(x=x, feet=feet, contact_state=contact, t_now=t_now, gait=gait, mass=mass,
                inertia_body=Ib, force=force, hip=hip)


# (B, seed) of every generator draw the GPU test steps on the device; tests/test_srb.py checks
# on the CPU that none of them puts a gait phase within 1e-9 of a boundary
ORACLE_CASES = [(1, 101), (255, 355), (256, 356), (257, 357), (513, 7)]
STRIDED_CASE = (257, 31)
PADDED_CASES = [(1, 41), (255, 295), (257, 297)]


def phase_margin(inp, h, nsub):
    """Smallest distance of any leg's gait phase from the duty boundary or the wrap at 0 / 1,
    over the start times of ``nsub`` substeps."""
    g, t, margin = inp["gait"], inp["t_now"].copy(), np.inf
    for _ in range(nsub):
        ph = np.mod(g[:, 2:6] + (t / g[:, 0])[:, None], 1.0)
        margin = min(margin, np.abs(ph - g[:, 1:2]).min(), ph.min(), (1.0 - ph).min())
        t = t + h
    return float(margin)


ARGS = ("x", "feet", "contact_state", "t_now", "gait", "mass", "inertia_body", "force", "hip")


def oracle(inp, h, nsub, dtype=np.float64, model=srb_ref.Plant):
    return srb_ref.srb_step(*(inp[k] for k in ARGS), h, nsub, dtype=dtype, model=model)


def group_diff(a, b):
    """max |a - b| per state group of two (x, feet, contact) results."""
    xa, xb = np.asarray(a[0], np.float64), np.asarray(b[0], np.float64)
    d = {g: float(np.abs(xa[:, s] - xb[:, s]).max(initial=0.0)) for g, s in _SLICE.items()}
    d["feet"] = float(np.abs(np.asarray(a[1], np.float64) - np.asarray(b[1], np.float64))
                      .max(initial=0.0))
    return d


def group_scale(r):
    x = np.asarray(r[0], np.float64)
    d = {g: float(np.abs(x[:, s]).max(initial=0.0)) for g, s in _SLICE.items()}
    d["feet"] = float(np.abs(np.asarray(r[1], np.float64)).max(initial=0.0))
    return d


def yardstick(inp, h, nsub):
    """(oracle64 result, oracle32 result, d_g = max |oracle32 - oracle64| per group)."""
    r64 = oracle(inp, h, nsub)
    r32 = oracle(inp, h, nsub, dtype=np.float32)
    return r64, r32, group_diff(r32, r64)


def tolerances(r64, d):
    """|device - oracle64| <= 8 d_g + 4 * 2^-24 * max |oracle64_g| per group."""
    sc = group_scale(r64)
    return {g: 8.0 * d[g] + 4.0 * EPS32 * sc[g] for g in GROUPS}


def check_against_oracle(got, inp, h, nsub, label=""):
    """``got`` = (x, feet, contact) from the device: contact bits exact, feet of legs that did
    not land bit-identical to the input, landed feet at z == 0 exactly, every group within the
    tolerance.  Prints and returns the per-group ratio (device error) / (float32 yardstick)."""
    r64, r32, d = yardstick(inp, h, nsub)
    np.testing.assert_array_equal(r32[2], r64[2])      # the yardstick saw the same contacts
    x, feet, contact = got
    np.testing.assert_array_equal(np.asarray(contact), r64[2])
    feet = np.asarray(feet).reshape(-1, 4, 3)
    feet_in = np.asarray(inp["feet"], np.float32).reshape(-1, 4, 3)
    landed = np.any(r64[1] != np.asarray(inp["feet"], np.float64).reshape(-1, 4, 3), axis=2)
    assert np.array_equal(feet[~landed], feet_in[~landed])
    assert np.all(feet[landed][:, 2] == 0.0)
    err, tol = group_diff((x, feet), r64), tolerances(r64, d)
    ratio = {g: (err[g] / d[g] if d[g] > 0 else 0.0) for g in GROUPS}
    print(f"{label} landed legs {int(landed.sum())}; device error / float32 yardstick: "
          + ", ".join(f"{g} {ratio[g]:.2f} ({err[g]:.2e} / {d[g]:.2e})" for g in GROUPS))
    for g in GROUPS:
        assert err[g] <= tol[g], (label, g, err[g], tol[g], d[g])
    return ratio
