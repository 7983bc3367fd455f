"""CPU: the reference for the derivatives of the rigid-body plant (tests/srb_grad_util.py) checked
against itself and against finite differences, the cases the GPU test uses checked for what they
cover, and the ctypes mirrors of the two io structs checked against the header.

Measured here: the direction check is at most 2.3e-15 x S at nsub = 20 and 5.4e-15 x S at
nsub = 64, so the reference's own noise stays 100 x under the device's bar of 1e-12 x S; the
central differences are within 1.3e-8 (1 + |J|) of J, whose largest entry is 203."""
import ctypes
import re

import numpy as np
import pytest

import srb_grad_util as sg
import srb_util
from conftest import REPO


@pytest.mark.parametrize("B,seed,nsub", sg.CASES)
def test_jacobian_against_one_run_along_the_direction(B, seed, nsub):
    """J d from 46 unit runs against one complex-step run along d itself, within 1e-14 x S: the
    two differ by the roundings of 46 separate runs and a sum, no more."""
    inp, _, d = sg.case(B, seed, nsub)
    J = sg.jacobian(inp, sg.H, nsub)
    (vals, S), direct = sg.ref_jvp(J, d), sg.split(sg.complex_step(inp, sg.H, nsub, d), sg.OUTPUTS)
    worst = sg.worst_ratio(direct, vals, S, tol=1e-14)
    print(f"B={B} seed={seed} nsub={nsub} worst |J d - run along d| / (1e-14 S):", worst)
    assert np.all(np.isfinite(J)) and max(worst.values()) <= 1.0, worst


def test_real_part_is_the_float64_run():
    """The complex run takes the float64 run's branches: the contact bits are that run's exactly,
    and its real part is that run's up to the different roundings of complex products and
    quotients -- 64 substeps of ~100 operations of 2^-53 each: within 1e-12 (1 + |value|)."""
    from oracle import srb_ref
    B, seed, nsub = sg.NSUB_CASES[-1]
    inp, _, d = sg.case(B, seed, nsub)
    moved = dict(inp)
    for n, t in sg.split(d).items():
        moved[n] = np.asarray(inp[n], np.float64).reshape(t.shape) + 1j * sg.STEP * t
    xc, fc, cc = srb_ref.srb_step(*(moved[k] for k in srb_util.ARGS), sg.H, nsub, dtype=np.complex128)
    x, f, c = srb_util.oracle(inp, sg.H, nsub)
    assert np.array_equal(cc, c)
    assert np.all(np.abs(xc.real - x) <= 1e-12 * (1.0 + np.abs(x)))
    assert np.all(np.abs(fc.real - f) <= 1e-12 * (1.0 + np.abs(f)))
    assert np.all(np.abs(xc.imag) < 1e-26) and np.all(np.abs(fc.imag) < 1e-26)


def test_jacobian_against_central_differences():
    """J against central differences of the float64 oracle with a step of 1e-6.  The bar is the
    difference's own error: rounding, 2^-53 |f| amplified by the ~10 nsub operations of a run and
    divided by the step -- 1.1e-16 x 4 x 200 / 1e-6 = 9e-8 for outputs up to 4 (a yaw) -- plus
    truncation, step^2 / 6 times a third derivative, which for entries up to ~100 whose scale of
    variation is ~0.1 (an inertia entry) is 1e-12 x 100 / 1e-3 / 6 = 2e-8.  Assert 1e-7 (1 + |J|)."""
    B, seed, nsub = sg.MAIN
    inp, _, _ = sg.case(B, seed, nsub)
    J = sg.jacobian(inp, sg.H, nsub)
    step, worst = 1e-6, 0.0
    flat = lambda r: np.concatenate([r[0], r[1].reshape(B, 12)], 1)          # noqa: E731
    for j in range(sg.NIN):
        e = np.zeros((B, sg.NIN))
        e[:, j] = step
        out = []
        for sign in (1.0, -1.0):
            moved = dict(inp)
            for n, t in sg.split(sign * e).items():
                moved[n] = np.asarray(inp[n], np.float64).reshape(t.shape) + t
            out.append(flat(srb_util.oracle(moved, sg.H, nsub)))
        fd = (out[0] - out[1]) / (2 * step)
        worst = max(worst, float((np.abs(fd - J[:, :, j]) / (1.0 + np.abs(J[:, :, j]))).max()))
    print("worst |central difference - J| / (1 + |J|):", worst, " max |J|:", float(np.abs(J).max()))
    assert worst <= 1e-7


@pytest.mark.parametrize("B,seed,nsub", sg.CASES)
def test_phase_margin_of_the_gpu_cases(B, seed, nsub):
    inp, _, _ = sg.case(B, seed, nsub)
    margin = srb_util.phase_margin(inp, sg.H, nsub)
    print(f"B={B} seed={seed} nsub={nsub} phase margin {margin:.2e}")
    assert margin >= 1e-9


def test_contact_coverage_of_the_gpu_cases():
    """Between them the cases hold a leg that lands at the first substep, one that lands later,
    one that lifts, one in swing throughout, and the constructed lift-then-land."""
    first = later = lifts = swing = lift_land = 0
    for B, seed, nsub in sg.CASES:
        st = sg.schedule(sg.case(B, seed, nsub)[0], sg.H, nsub)
        land, lift = st[:, 1:] & ~st[:, :-1], ~st[:, 1:] & st[:, :-1]
        first += int(land[:, 0].sum())
        later += int(land[:, 1:].sum())
        lifts += int(lift.sum())
        swing += int((~st).all(1).sum())
        k_lift = np.where(lift.any(1), lift.argmax(1), nsub)
        k_land = np.where(land.any(1), nsub - 1 - land[:, ::-1].argmax(1), -1)
        lift_land += int((k_lift < k_land).sum())
    print(f"landings at the first substep {first}, later {later}; lifts {lifts}; legs in swing "
          f"throughout {swing}; lift-then-land {lift_land}")
    assert min(first, later, lifts, swing, lift_land) >= 1
    st = sg.schedule(sg.constructed_robot(), sg.H, 64)[0]
    assert st[:6, 0].all() and not st[6:54, 0].any() and st[54:, 0].all()  # lifts at 5, lands at 53


def _c_layout(name):
    """Field -> (offset, size) and the sizeof of struct ``name`` as include/cmpc.h declares it, by
    the C rules for an LP64 target (every field here is a pointer or a fixed-width scalar)."""
    h = (REPO / "include" / "cmpc.h").read_text()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, re.S).group(1)
    sizes = dict(uint32_t=4, int32_t=4, int64_t=8, double=8, float=4, uint8_t=1)
    at, out, widest = 0, {}, 1
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)$", decl)
        size = 8 if m.group(2) else sizes[m.group(1)]
        at = (at + size - 1) // size * size
        out[m.group(3)] = (at, size)
        at, widest = at + size, max(widest, size)
    return out, (at + widest - 1) // widest * widest


@pytest.mark.parametrize("struct,mirror", [("cmpc_srb_vjp_io", "CSrbVjpIO"),
                                           ("cmpc_srb_jvp_io", "CSrbJvpIO")])
def test_struct_mirrors(struct, mirror):
    from cmpc import _lib
    m = getattr(_lib, mirror)
    fields, size = _c_layout(struct)
    assert [n for n, _ in m._fields_] == list(fields)
    for n, (offset, width) in fields.items():
        assert (getattr(m, n).offset, getattr(m, n).size) == (offset, width), n
    assert ctypes.sizeof(m) == size == 160
    # and by hand
    assert (m.size.offset, m.t_now.offset, m.force_stride.offset, m.contact_state.offset) == (0, 8, 48, 80)
    assert (m.nsub.offset, m.dt.offset) == (88, 96)
    first = dict(CSrbVjpIO="g_x", CSrbJvpIO="d_x_out")[mirror]
    assert getattr(m, first).offset == dict(CSrbVjpIO=120, CSrbJvpIO=144)[mirror]
    assert _lib.SRB_VJP_OUTPUTS == _lib.SRB_JVP_TANGENTS == sg.INPUTS
    assert _lib.SRB_JVP_OUTPUTS == sg.OUTPUTS
    assert ("#define CMPC_SRB_GRAD_MAX_NSUB %d" % _lib.SRB_GRAD_MAX_NSUB) in (
        REPO / "include" / "cmpc.h").read_text()
    assert "cmpc_srb_vjp_run" in _lib.EXPORTS and "cmpc_srb_jvp_run" in _lib.EXPORTS
