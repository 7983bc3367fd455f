"""Shared by tests/test_srb_grad.py (CPU) and tests/test_gpu_srb_grad.py (TEST INFRASTRUCTURE):
the reference for the derivatives of the rigid-body plant (cmpc_srb_vjp_run / cmpc_srb_jvp_run,
include/cmpc.h) and the cases both files use.

The reference is complex-step differentiation of the unmodified oracle: ``oracle/srb_ref.srb_step``
runs as it stands with ``dtype=np.complex128``, and with a step of 1e-30 along a real direction d
the real part of its result is the float64 run and the imaginary part over 1e-30 is the
directional derivative, with no truncation and no cancellation error.  The contact schedule is
read off float64 times and gait, which stay real, so the complex run takes the float64 run's
branches.  46 unit directions give the Jacobian J (B, 24, 46) -- outputs x' (12) then feet' (12),
inputs x (12), feet (12), force (12), mass (1), inertia_body (9) -- and

  ref_jvp = J d   with the scale S = |J| |d|      per robot and output entry,
  ref_vjp = J' g  with the scale S = |J|' |g|     per robot and input entry:

S is what the result would be without any cancellation between its terms, the quantity a
rounding-error bound is proportional to.  An entry with S == 0 has no term at all.
"""
from __future__ import annotations

import functools

import numpy as np

import srb_util
from oracle import srb_ref

STEP = 1e-30
TOL = 1e-12          # device against the reference, x S (dyn_grad_util.TOL)
REL32 = 2.0 ** -23   # one fp32 rounding of the jvp's fp32 outputs
H = srb_util.H
INPUTS = ("x", "feet", "force", "mass", "inertia_body")      # the inputs that move
SIZES = dict(x=12, feet=12, force=12, mass=1, inertia_body=9)
SHAPES = dict(x=(12,), feet=(4, 3), force=(12,), mass=(), inertia_body=(3, 3))
OUTPUTS = ("x", "feet")
NIN, NOUT = 46, 24

# (B, seed, nsub) of every draw the GPU test differentiates on the device; test_srb_grad.py checks
# on the CPU that none puts a gait phase within 1e-9 of a boundary.  The nsub of the second group
# straddle the vjp kernel's segment length of 8 and the threshold of 24 between its short-tape and
# long-tape instantiations; its nsub = 64 case carries the constructed robot.
BATCH_CASES = [(1, 101, 20), (63, 163, 20), (64, 164, 20), (65, 165, 20), (257, 357, 20)]
NSUB_CASES = [(67, 7, n) for n in (1, 7, 8, 9, 20, 24, 25, 64)]
CASES = BATCH_CASES + NSUB_CASES
MAIN = (67, 7, 20)


def constructed_robot() -> dict:
    """One robot whose leg 0 lifts at substep 5 and lands again at substep 53 of 64 substeps of H:
    period 0.25 and duty 0.8 make a swing of 0.05 s = 48 substeps, t_now = 0 makes the phase
    offset + k / 240, and offset 0.8 - 4.5 / 240 puts both crossings half a substep (2e-3 of
    phase) from a substep's start.  Leg 1 stays in stance, leg 2 lands at substep 24 and leg 3
    lifts at substep 37."""
    inp = srb_util.make_plant_inputs(1, 9001)
    inp["t_now"] = np.zeros(1)
    inp["gait"] = np.array([[0.25, 0.8, 0.8 - 4.5 / 240, 0.1, 0.9 + 0.5 / 240, 0.65 - 0.5 / 240]])
    g = inp["gait"]
    inp["contact_state"] = srb_util.mask_bits(
        srb_ref.stance_mask(inp["t_now"] - H, g[:, 0], g[:, 1], g[:, 2:6]))
    return inp


def concat(a: dict, b: dict) -> dict:
    """Two batches of plant inputs as one (hip is shared)."""
    return {k: (a[k] if k == "hip" else np.concatenate([a[k], b[k]], 0)) for k in a}


@functools.lru_cache(maxsize=None)
def case(B, seed, nsub):
    """-> (inputs, gradients g (rows, 24), tangents d (rows, 46)) of a case, computed once and
    shared (not modified).  Gradients and tangents are standard normal.  nsub = 64 appends the
    constructed robot, so that case has B + 1 rows."""
    inp = srb_util.make_plant_inputs(B, seed)
    if nsub == 64:
        inp = concat(inp, constructed_robot())
    rows = inp["x"].shape[0]
    rng = np.random.default_rng(100000 + 1000 * nsub + seed)
    g = rng.standard_normal((rows, NOUT))
    d = srb_util.f32(rng.standard_normal((rows, NIN)))      # (the entry's tangents are fp32)
    return inp, g, d


def schedule(inp, h, nsub):
    """-> stance (B, nsub + 1, 4) bool: row 0 is contact_state, row k + 1 the mask at substep k."""
    g, t = inp["gait"], np.array(inp["t_now"], np.float64)
    rows = [srb_util.bits_mask(inp["contact_state"])]
    for _ in range(nsub):
        rows.append(srb_ref.stance_mask(t, g[:, 0], g[:, 1], g[:, 2:6]))
        t = t + h
    return np.stack(rows, 1)


def split(v, names=INPUTS):
    """(B, sum of sizes) -> name -> array of the input's shape."""
    out, at = {}, 0
    for n in names:
        out[n] = v[:, at:at + SIZES[n]].reshape((v.shape[0],) + SHAPES[n])
        at += SIZES[n]
    return out


def complex_step(inp, h, nsub, d):
    """The directional derivative of (x', feet') along d (B, 46), one complex run -> (B, 24)."""
    B = inp["x"].shape[0]
    moved = dict(inp)
    for n, t in split(np.asarray(d, np.float64)).items():
        moved[n] = np.asarray(inp[n], np.float64).reshape(t.shape) + 1j * STEP * t
    x, feet, _ = srb_ref.srb_step(*(moved[k] for k in srb_util.ARGS), h, nsub, dtype=np.complex128)
    return np.concatenate([x, feet.reshape(B, 12)], 1).imag / STEP


def jacobian(inp, h, nsub):
    """J (B, 24, 46) from 46 unit-tangent complex-step runs."""
    B = inp["x"].shape[0]
    J = np.empty((B, NOUT, NIN))
    for j in range(NIN):
        d = np.zeros((B, NIN))
        d[:, j] = 1.0
        J[:, :, j] = complex_step(inp, h, nsub, d)
    return J


def ref_jvp(J, d):
    """-> (values, S), each name -> array over OUTPUTS."""
    v = np.einsum("boi,bi->bo", J, d)
    S = np.einsum("boi,bi->bo", np.abs(J), np.abs(d))
    return split(v, OUTPUTS), split(S, OUTPUTS)


def ref_vjp(J, g):
    """-> (values, S), each name -> array over INPUTS."""
    v = np.einsum("boi,bo->bi", J, g)
    S = np.einsum("boi,bo->bi", np.abs(J), np.abs(g))
    return split(v), split(S)


def worst_ratio(got, vals, S, tol=TOL, rel=0.0):
    """traj_grad_util.worst_ratio with S per entry: name -> max over robots and entries of
    |got - ref| / (rel |ref| + tol S) for the outputs present in got; where the bound is 0, 0 if
    got equals the reference (the sign of a zero apart), else inf."""
    out = {}
    for n, g in got.items():
        ref = np.asarray(vals[n], np.float64)
        g = np.asarray(g, np.float64).reshape(ref.shape)
        err = np.abs(g - ref)
        bound = rel * np.abs(ref) + tol * np.asarray(S[n]).reshape(ref.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))
        out[n] = float(r.max()) if r.size else 0.0
    return out
