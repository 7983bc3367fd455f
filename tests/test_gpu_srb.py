"""GPU: the rigid-body plant ``cmpc_srb_step`` (csrc/cmpc_sim.hip) against the float64 oracle
``oracle/srb_ref.py``, on the inputs of ``srb_util.make_plant_inputs`` (tilted, turning robots
with full inertias and per-robot gaits; tests/test_srb.py shows that these inputs separate the
documented model from eight plausible mistakes by at least 100 float32 yardsticks).

Tolerance, per state group g (p, rpy, v, w, feet): with d_g = max |oracle32 - oracle64| on the
same input, |device - oracle64| <= 8 d_g + 4 * 2^-24 * max |oracle64_g|.  The device's sinf /
cosf / division are accurate to a few ulp but not correctly rounded and FMA contraction changes
single roundings, so the kernel's error is of the order of the NumPy float32 error, not equal
to it.  Contact bits, feet that did not land and the z of feet that landed are exact.

Measured on an MI355X, the largest (device error) / d_g over all cases of this file:
  p 1.00, rpy 1.00, v 1.02, w 1.51, feet 2.67  (the bar is 8; the float32 rounding of h is a
  systematic part of d_g that the device shares, hence the many ratios of exactly 1.00).
With the sign of w x I_w w flipped, R and R' exchanged in I_w, the yaw rate without its
sp * roll-rate term, or p advanced with the old v in a scratch copy of the kernel, every
comparison of this file failed (ratios 102 to 720,000 on the single-robot, single-substep case).
"""
import ctypes

import numpy as np
import pytest

from srb_util import (H, ORACLE_CASES, PADDED_CASES, STRIDED_CASE, check_against_oracle,
                      make_plant_inputs, mask_bits)

pytestmark = pytest.mark.gpu

CMPC_OK, CMPC_E_INVALID = 0, -22
SENTINEL = 1e6


class _Call:
    """Device copies of one input set and the ctypes call ``ClosedLoop._tick`` makes."""

    def __init__(self, plan, inp, pad=0, force_buf=None, force_off=0):
        import torch
        self.torch, self.plan = torch, plan
        dev = plan.device
        B = self.B = len(inp["x"])
        f32, f64 = torch.float32, torch.float64

        def up(a, dtype):
            return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev).contiguous()

        def padded(a, dtype, fill):
            a = np.asarray(a).reshape(B, -1)
            full = np.full((B + pad, a.shape[1]), fill, a.dtype)
            full[:B] = a
            return up(full, dtype)
        self.x = padded(inp["x"], f32, SENTINEL)
        self.feet = padded(inp["feet"], f32, SENTINEL)
        self.contact = padded(inp["contact_state"], torch.uint8, 0xA5)
        self.t = up(inp["t_now"], f64)
        self.gait = up(inp["gait"], f64)
        self.mass = up(inp["mass"], f32)
        self.Ib = up(inp["inertia_body"], f32)
        self.hip = up(inp["hip"], f32)
        if force_buf is None:
            self.force, self.force_off = up(inp["force"], f32), 0
        else:
            self.force, self.force_off = up(force_buf, f32), force_off
        self.stride = self.force.shape[1]

    def step(self, h, nsub, B=None, stride=None):
        torch, p = self.torch, self.plan
        P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        fp = ctypes.c_void_p(self.force.data_ptr() + 4 * self.force_off)
        with torch.cuda.device(p.device):
            rc = p.lib.cmpc_srb_step(
                p._h, ctypes.c_int64(self.B if B is None else B), ctypes.c_int(nsub),
                ctypes.c_double(h), P(self.t), P(self.gait), P(self.mass), P(self.Ib), fp,
                ctypes.c_int64(self.stride if stride is None else stride), P(self.hip),
                P(self.x), P(self.feet), P(self.contact),
                ctypes.c_void_p(torch.cuda.current_stream(p.device).cuda_stream))
        torch.cuda.synchronize(p.device)
        return rc

    def result(self):
        return (self.x.cpu().numpy(), self.feet.cpu().numpy().reshape(-1, 4, 3),
                self.contact.cpu().numpy().reshape(-1))

    def rows(self, lo, hi):
        x, feet, c = self.result()
        return x[lo:hi], feet[lo:hi], c[lo:hi]


def _device_step(plan, inp, h, nsub, **kw):
    c = _Call(plan, inp, **kw)
    assert c.step(h, nsub) == CMPC_OK, plan.lib.cmpc_last_error().decode()
    return c


@pytest.mark.parametrize("nsub", [1, 20])
@pytest.mark.parametrize("B,seed", ORACLE_CASES, ids=[str(b) for b, _ in ORACLE_CASES])
def test_kernel_against_oracle(plan, B, seed, nsub):
    """The 256-thread block edge on both sides, one and three blocks, one robot."""
    inp = make_plant_inputs(B, seed)
    c = _device_step(plan, inp, H, nsub)
    check_against_oracle(c.result(), inp, H, nsub, label=f"B={B} nsub={nsub}:")


def test_events_happen_on_the_device(plan):
    """The 513-robot input at 20 substeps lands and lifts legs (tests/test_srb.py counts them on
    the CPU): the device's contact bits changed accordingly."""
    inp = make_plant_inputs(513, seed=7)
    c = _device_step(plan, inp, H, 20)
    before, after = inp["contact_state"], c.result()[2]
    assert np.sum((after & ~before) != 0) >= 32 and np.sum((before & ~after) != 0) >= 32


@pytest.mark.parametrize("nsub", [1, 20])
def test_strided_force_is_bit_identical(plan, nsub):
    """Forces read as the U[:, 0] rows of a (B, 384) solution buffer (offset 192, stride 384),
    the rest of each row a large sentinel: the same bits as the packed (B, 12) call."""
    B, seed = STRIDED_CASE
    inp = make_plant_inputs(B, seed)
    packed = _device_step(plan, inp, H, nsub).result()
    buf = np.full((B, 384), SENTINEL, np.float32)
    buf[:, 192:204] = inp["force"]
    strided = _device_step(plan, inp, H, nsub, force_buf=buf, force_off=192).result()
    for a, b in zip(packed, strided):
        assert np.array_equal(a, b)
    check_against_oracle(strided, inp, H, nsub, label=f"strided nsub={nsub}:")


@pytest.mark.parametrize("B,seed", PADDED_CASES, ids=[str(b) for b, _ in PADDED_CASES])
def test_rows_past_the_batch_are_untouched(plan, B, seed):
    """x, feet and contact_state carry 64 more rows of sentinel than the B passed."""
    inp = make_plant_inputs(B, seed)
    c = _device_step(plan, inp, H, 20, pad=64)
    x, feet, contact = c.result()
    assert x.shape[0] == B + 64
    assert np.all(x[B:] == np.float32(SENTINEL)) and np.all(feet[B:] == np.float32(SENTINEL))
    assert np.all(contact[B:] == 0xA5)
    check_against_oracle(c.rows(0, B), inp, H, 20, label=f"padded B={B}:")


def test_large_times_and_exact_phase_ties(plan):
    """Two blocks outside the generator's 1e-9 phase margin: times near 1e3 with a shared trot,
    and exact ties (duty 1/2, t_now a multiple of period / 16, phase == duty at the start).
    Both sides evaluate the phase in float64 in the same order: the bits still agree."""
    from oracle import srb_ref
    B = 512
    inp = make_plant_inputs(B, seed=52)
    period = 1.0 / 3
    g, t = inp["gait"], inp["t_now"]
    g[:256] = np.array([period, 0.5, 0.5, 0.0, 0.0, 0.5])
    t[:256] = np.arange(256) * (period / 16)
    g[256:, 0] = period
    t[256:] = 1000.0 + np.arange(256) * (period / 16) * 0.5
    inp["contact_state"] = mask_bits(srb_ref.stance_mask(t - H, g[:, 0], g[:, 1], g[:, 2:6]))
    ph = np.mod(g[:256, 2:6] + (t[:256] / g[:256, 0])[:, None], 1.0)
    assert np.sum(ph == 0.5) >= 32               # the ties are there
    for nsub in (1, 20):
        c = _device_step(plan, inp, H, nsub)
        check_against_oracle(c.result(), inp, H, nsub, label=f"ties/late nsub={nsub}:")


def test_early_returns_and_invalid_arguments(plan):
    inp = make_plant_inputs(16, seed=60)
    c = _Call(plan, inp)
    before = c.result()
    assert c.step(H, 0) == CMPC_OK
    assert c.step(H, 20, B=0) == CMPC_OK
    for a, b in zip(before, c.result()):
        assert np.array_equal(a, b)
    for kw, h in ((dict(stride=11), H), ({}, 0.0), ({}, float("nan"))):
        assert c.step(h, 20, **kw) == CMPC_E_INVALID
        assert "cmpc_srb_step" in plan.lib.cmpc_last_error().decode()
    for a, b in zip(before, c.result()):
        assert np.array_equal(a, b)
