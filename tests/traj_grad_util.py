"""Shared helpers of the cmpc_traj_vjp_run / cmpc_traj_jvp_run tests (TEST INFRASTRUCTURE, float64
NumPy on the fp32-rounded inputs that the device receives): the smooth function that
cmpc_generate_traj evaluates before it rounds, its reverse- and forward-mode derivatives written
out from the formulas of include/cmpc.h over the whole batch, and the scale S of every output.

Per robot, with (px, py, phi, theta, psi) = x0[0, 1, 3, 4, 5], (vxb, vyb, zdes, wz) = cmd,
t_k = (k + 1) dt and tau = ((1 - duty) period + 0.5 duty period) / 2:
  clamp   sigma_a = 1 where the forward pass clamps axis a (strict tests, its order), pd_a = p_a +- 0.1
          there and pos_des[a] elsewhere, pd_z = zdes
  xref[k] = (pd_x + vwx t_k, pd_y + vwy t_k, pd_z, 0, 0, psi + wz t_k, vwx, vwy, 0, 0, 0, wz),
          vwx = c vxb - s vyb, vwy = s vxb + c vyb  (c, s of psi)
  lever of (k, leg): class S (swing at the step's start) 0; class C (stance, no take-off at a
          step <= k) foot_lever[leg]; class P (stance, last take-off at step j <= k)
          (hwx + vbx tau - wz tau hwy, hwy + vby tau + wz tau hwx, 0.02 - zdes) with
          (hwx, hwy) = R_z(psi + wz t_j) hip[leg] and (vbx, vby) the body-frame velocity.
The contact pattern (the classes and j) depends on t_now and gait alone and is held fixed.

Scale S per output and robot: the defining formula with every factor replaced by its absolute
value and every difference by a sum, through the intermediates as well, the largest entry of the
robot's part of that output.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

VJP_OUTPUTS = ("x0", "pos_des", "cmd", "foot_lever")
JVP_TANGENTS = ("x0", "pos_des", "cmd", "foot_lever")
JVP_OUTPUTS = ("xref", "r_feet", "pos_des")
INPUTS = ("x0", "pos_des", "cmd", "t_now", "gait", "hip")
TOL = 1e-12         # device against the reference, x S
REL32 = 2.0 ** -23  # one fp32 rounding of the jvp's fp32 outputs
MAX_POS_ERROR = 0.1
TD_HEIGHT = 0.02
SWING, CURRENT, PREDICTED = 0, 1, 2


def f32(a):
    """The array as the device receives it: rounded to fp32, widened exactly."""
    return np.asarray(np.asarray(a, np.float32), np.float64)


def classes(t_now, gait, dt, N):
    """-> cls (B, N, 4) in {SWING, CURRENT, PREDICTED}, j (B, N, 4) the last take-off step of a
    PREDICTED lever (-1 elsewhere): the stance mask at the start of every step
    (mod(offset + t / period, 1) < duty, float64, the forward pass's operation order), a take-off
    where a leg is in swing and was in stance the step before (or the step is the first)."""
    t_now, gait = np.asarray(t_now, np.float64), np.asarray(gait, np.float64)
    B = len(t_now)
    period, duty, offs = gait[:, 0], gait[:, 1], gait[:, 2:6]
    t = t_now[:, None] + np.arange(N)[None, :] * dt
    mask = np.mod(offs[:, :, None] + t[:, None, :] / period[:, None, None], 1.0) < duty[:, None, None]
    cls = np.zeros((B, N, 4), int)
    jj = np.full((B, N, 4), -1)
    last = np.full((B, 4), -1)
    prev = np.ones((B, 4), bool)
    for k in range(N):
        m = mask[:, :, k]
        last = np.where(~m & prev, k, last)
        cls[:, k] = np.where(~m, SWING, np.where(last < 0, CURRENT, PREDICTED))
        jj[:, k] = np.where(m & (last >= 0), last, -1)
        prev = m
    return cls, jj


def _leaves(x0, pos_des, cmd, t_now, gait, hip, dt, N):
    """The primal quantities both derivatives read, as a namespace of float64 arrays: per robot
    (B,), per step (1, N) and per (step, leg) (B, N, 4)."""
    x0, cmd, hip = f32(x0), f32(cmd), f32(hip)
    pos_des, gait = np.asarray(pos_des, np.float64), np.asarray(gait, np.float64)
    B = x0.shape[0]
    q = SimpleNamespace(B=B, N=N, dt=float(dt))
    q.p = x0[:, 0:2]
    q.vxb, q.vyb, q.zdes, q.wz = cmd[:, 0], cmd[:, 1], cmd[:, 2], cmd[:, 3]
    phi, theta, q.psi = x0[:, 3], x0[:, 4], x0[:, 5]
    q.c, q.s = np.cos(q.psi), np.sin(q.psi)
    q.cph, q.sph, q.cth, q.sth = np.cos(phi), np.sin(phi), np.cos(theta), np.sin(theta)
    pd = pos_des.copy()
    q.sigma = np.zeros((B, 2))
    for a in range(2):                                    # the forward pass's tests, in its order
        cur = q.p[:, a]
        hi = pd[:, a] - cur > MAX_POS_ERROR
        pd[hi, a] = cur[hi] + MAX_POS_ERROR
        lo = cur - pd[:, a] > MAX_POS_ERROR
        pd[lo, a] = cur[lo] - MAX_POS_ERROR
        q.sigma[:, a] = hi | lo
    pd[:, 2] = q.zdes
    q.pd = pd
    period, duty = gait[:, 0], gait[:, 1]
    q.tau = ((1.0 - duty) * period + 0.5 * (duty * period)) / 2.0
    q.tk = ((np.arange(N) + 1) * q.dt)[None, :]
    q.cls, jj = classes(t_now, gait, q.dt, N)
    q.P, q.C = (q.cls == PREDICTED) * 1.0, (q.cls == CURRENT) * 1.0
    q.tj = (jj + 1) * q.dt * q.P
    psij = q.psi[:, None, None] + q.wz[:, None, None] * q.tj
    q.cj, q.sj = np.cos(psij) * q.P, np.sin(psij) * q.P   # (zero outside class P, as hwx, hwy)
    q.hx, q.hy = hip[None, None, :, 0], hip[None, None, :, 1]
    return q


def _derived(q, m):
    """The intermediates from the leaves; m = -1: the values, m = +1 (on leaves made absolute):
    their scales."""
    q.vwx = q.c * q.vxb + m * q.s * q.vyb
    q.vwy = q.s * q.vxb + q.c * q.vyb
    q.hwx = q.cj * q.hx + m * q.sj * q.hy
    q.hwy = q.sj * q.hx + q.cj * q.hy
    return q


def _absolute(q):
    """The leaves with every factor made absolute."""
    r = SimpleNamespace(**vars(q))
    for n in ("vxb", "vyb", "zdes", "wz", "c", "s", "cph", "sph", "cth", "sth", "cj", "sj", "hx",
              "hy", "p", "pd", "psi"):
        setattr(r, n, np.abs(getattr(q, n)))
    return r


def _b(v):
    return v[:, None, None]


def _forward_core(q, fl, m):
    vbx = (q.c * q.cth) * q.vwx + (q.s * q.cth) * q.vwy
    vby = (q.c * q.sth * q.sph + m * q.s * q.cph) * q.vwx + (q.s * q.sth * q.sph + q.c * q.cph) * q.vwy
    xref = np.zeros((q.B, q.N, 12))
    xref[:, :, 0] = q.pd[:, 0:1] + q.vwx[:, None] * q.tk
    xref[:, :, 1] = q.pd[:, 1:2] + q.vwy[:, None] * q.tk
    xref[:, :, 2] = q.pd[:, 2:3]
    xref[:, :, 5] = q.psi[:, None] + q.wz[:, None] * q.tk
    xref[:, :, 6], xref[:, :, 7], xref[:, :, 11] = q.vwx[:, None], q.vwy[:, None], q.wz[:, None]
    tau, wz = _b(q.tau), _b(q.wz)
    r = np.stack([q.hwx + _b(vbx) * tau + m * wz * tau * q.hwy,
                  q.hwy + _b(vby) * tau + wz * tau * q.hwx,
                  np.broadcast_to(TD_HEIGHT + m * _b(q.zdes), q.P.shape)], -1) * q.P[..., None]
    r = r + fl[:, None] * q.C[..., None]
    return dict(xref=xref, r_feet=r, pos_des=q.pd.copy())


def _rowmax(v, B):
    return np.abs(v).reshape(B, -1).max(axis=1)


def forward(x0, pos_des, cmd, t_now, gait, foot_lever, hip, dt, N):
    """The smooth function -> (vals, S, cls): vals and S dicts over ("xref", "r_feet", "pos_des")
    (pos_des the value after the clamp), cls (B, N, 4) the lever classes."""
    q = _leaves(x0, pos_des, cmd, t_now, gait, hip, dt, N)
    fl = f32(foot_lever)
    vals = _forward_core(_derived(q, -1.0), fl, -1.0)
    sc = _forward_core(_derived(_absolute(q), 1.0), np.abs(fl), 1.0)
    return vals, {n: _rowmax(v, q.B) for n, v in sc.items()}, q.cls


def _jvp_core(q, d_x0, d_pd, d_cmd, d_fl, m):
    dp, dphi, dth, dpsi = d_x0[:, 0:2], d_x0[:, 3], d_x0[:, 4], d_x0[:, 5]
    dvx, dvy, dz, dwz = d_cmd[:, 0], d_cmd[:, 1], d_cmd[:, 2], d_cmd[:, 3]
    dvwx = q.c * dvx + m * q.s * dvy + m * q.vwy * dpsi
    dvwy = q.s * dvx + q.c * dvy + q.vwx * dpsi
    dpd = q.sigma * dp + (1.0 - q.sigma) * d_pd[:, 0:2]
    dx = np.zeros((q.B, q.N, 12))
    dx[:, :, 0] = dpd[:, 0:1] + dvwx[:, None] * q.tk
    dx[:, :, 1] = dpd[:, 1:2] + dvwy[:, None] * q.tk
    dx[:, :, 2] = dz[:, None]
    dx[:, :, 5] = dpsi[:, None] + dwz[:, None] * q.tk
    dx[:, :, 6], dx[:, :, 7], dx[:, :, 11] = dvwx[:, None], dvwy[:, None], dwz[:, None]
    dvbx = q.cth * dvx + m * q.sth * q.vxb * dth
    dvby = ((q.cth * q.sph * dth + q.sth * q.cph * dphi) * q.vxb + q.sth * q.sph * dvx +
            m * q.sph * q.vyb * dphi + q.cph * dvy)
    tau, wz = _b(q.tau), _b(q.wz)
    dpsij = _b(dpsi) + _b(dwz) * q.tj
    dhwx, dhwy = m * q.hwy * dpsij, q.hwx * dpsij
    dr = np.stack([dhwx + tau * _b(dvbx) + m * tau * (_b(dwz) * q.hwy + wz * dhwy),
                   dhwy + tau * _b(dvby) + tau * (_b(dwz) * q.hwx + wz * dhwx),
                   np.broadcast_to(m * _b(dz), q.P.shape)], -1) * q.P[..., None]
    dr = dr + d_fl[:, None] * q.C[..., None]
    return dict(xref=dx, r_feet=dr, pos_des=np.concatenate([dpd, dz[:, None]], 1))


def ref_jvp(x0, pos_des, cmd, t_now, gait, hip, dt, N, d_x0=None, d_pos_des=None, d_cmd=None,
            d_foot_lever=None):
    """-> (vals, S): dicts over JVP_OUTPUTS; vals float64 of the outputs' shapes, S (B,) each."""
    q = _leaves(x0, pos_des, cmd, t_now, gait, hip, dt, N)
    B = q.B
    d = [np.zeros((B, 12)) if d_x0 is None else f32(d_x0),
         np.zeros((B, 3)) if d_pos_des is None else np.asarray(d_pos_des, np.float64),
         np.zeros((B, 4)) if d_cmd is None else f32(d_cmd),
         np.zeros((B, 4, 3)) if d_foot_lever is None else f32(d_foot_lever)]
    vals = _jvp_core(_derived(q, -1.0), *d, -1.0)
    sc = _jvp_core(_derived(_absolute(q), 1.0), *[np.abs(t) for t in d], 1.0)
    return vals, {n: _rowmax(v, B) for n, v in sc.items()}


def _vjp_core(q, G, H, gp, m):
    s12 = lambda v: v.sum(axis=(1, 2))                                       # noqa: E731
    tau, wz = _b(q.tau), _b(q.wz)
    H0, H1, H2 = (H[..., i] * q.P for i in range(3))
    g_pd = G[:, :, 0:2].sum(1) + gp[:, 0:2]
    g_z = G[:, :, 2].sum(1) + gp[:, 2] + m * s12(H2)
    g_vwx = (q.tk * G[:, :, 0] + G[:, :, 6]).sum(1)
    g_vwy = (q.tk * G[:, :, 1] + G[:, :, 7]).sum(1)
    g_psi = G[:, :, 5].sum(1)
    g_wz = (q.tk * G[:, :, 5] + G[:, :, 11]).sum(1)
    g_vbx, g_vby = s12(tau * H0), s12(tau * H1)
    g_hwx, g_hwy = H0 + wz * tau * H1, H1 + m * wz * tau * H0
    g_wz = g_wz + s12(tau * (m * q.hwy * H0 + q.hwx * H1))
    g_pj = m * q.hwy * g_hwx + q.hwx * g_hwy
    g_psi = g_psi + s12(g_pj)
    g_wz = g_wz + s12(q.tj * g_pj)
    g_fl = (H * q.C[..., None]).sum(1)
    g_vxb = q.c * g_vwx + q.s * g_vwy + q.cth * g_vbx + q.sth * q.sph * g_vby
    g_vyb = m * q.s * g_vwx + q.c * g_vwy + q.cph * g_vby
    g_psi = g_psi + m * q.vwy * g_vwx + q.vwx * g_vwy
    g_th = m * q.sth * q.vxb * g_vbx + q.cth * q.sph * q.vxb * g_vby
    g_ph = (q.sth * q.cph * q.vxb + m * q.sph * q.vyb) * g_vby
    g_x0 = np.zeros((q.B, 12))
    g_x0[:, 0:2] = q.sigma * g_pd
    g_x0[:, 3], g_x0[:, 4], g_x0[:, 5] = g_ph, g_th, g_psi
    g_pos = np.concatenate([(1.0 - q.sigma) * g_pd, np.zeros((q.B, 1))], 1)
    return dict(x0=g_x0, pos_des=g_pos, cmd=np.stack([g_vxb, g_vyb, g_z, g_wz], 1), foot_lever=g_fl)


def ref_vjp(x0, pos_des, cmd, t_now, gait, hip, dt, N, g_xref=None, g_r_feet=None, g_yaw=None,
            g_pos_des=None):
    """-> (vals, S): dicts over VJP_OUTPUTS; vals float64 of the outputs' shapes, S (B,) each.
    ``pos_des`` is the value before the forward pass clamped it; ``g_pos_des`` is the gradient in
    the value after."""
    q = _leaves(x0, pos_des, cmd, t_now, gait, hip, dt, N)
    B = q.B
    G = np.zeros((B, N, 12)) if g_xref is None else np.array(g_xref, np.float64)
    aG = np.abs(G)
    if g_yaw is not None:
        G[:, :, 5] += (np.asarray(g_yaw, np.float64) / N)[:, None]
        aG[:, :, 5] += (np.abs(g_yaw) / N)[:, None]
    H = np.zeros((B, N, 4, 3)) if g_r_feet is None else np.asarray(g_r_feet, np.float64)
    gp = np.zeros((B, 3)) if g_pos_des is None else np.asarray(g_pos_des, np.float64)
    vals = _vjp_core(_derived(q, -1.0), G, H, gp, -1.0)
    sc = _vjp_core(_derived(_absolute(q), 1.0), aG, np.abs(H), np.abs(gp), 1.0)
    return vals, {n: _rowmax(v, B) for n, v in sc.items()}


def worst_ratio(got, vals, S, tol=TOL, rel=0.0):
    """name -> max over robots and entries of |got - ref| / (rel |ref| + tol S_robot) for the
    outputs present in got; where the bound is 0, 0 if got equals the reference, else inf."""
    out = {}
    for n, g in got.items():
        ref = np.asarray(vals[n], np.float64)
        g = np.asarray(g, np.float64).reshape(ref.shape)
        B = ref.shape[0]
        err = np.abs(g - ref).reshape(B, -1)
        bound = rel * np.abs(ref).reshape(B, -1) + tol * np.asarray(S[n])[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))
        out[n] = float(r.max()) if r.size else 0.0
    return out


def random_case(rng, B, N):
    """The tick inputs of synth.make_tick_inputs(B, seed=1000 N + B, mixed=True, N=N) as the
    device receives them, with standard-normal fp64 gradients and tangents (fp32 where the entry
    takes fp32)."""
    from cmpc import synth
    t = synth.make_tick_inputs(B, seed=1000 * N + B, mixed=True, N=N)
    c = dict(x0=np.float32(t["x0"]), pos_des=np.ascontiguousarray(t["pos_des"], np.float64),
             cmd=np.float32(t["cmd"]), t_now=np.asarray(t["t_now"], np.float64), gait=np.asarray(t["gait"], np.float64),
             foot_lever=np.float32(t["foot_lever"]), hip=np.float32(t["hip"]), dt=float(t["dt"]),
             N=N)
    c["g_xref"] = rng.standard_normal((B, N, 12))
    c["g_r_feet"] = rng.standard_normal((B, N, 4, 3))
    c["g_yaw"] = rng.standard_normal(B)
    c["g_pos_des"] = rng.standard_normal((B, 3))
    c["d_x0"] = np.float32(rng.standard_normal((B, 12)))
    c["d_pos_des"] = rng.standard_normal((B, 3))
    c["d_cmd"] = np.float32(rng.standard_normal((B, 4)))
    c["d_foot_lever"] = np.float32(rng.standard_normal((B, 4, 3)))
    return c


def inputs(c):
    """The positional inputs of ref_vjp / ref_jvp."""
    return [c[k] for k in INPUTS] + [c["dt"], c["N"]]


def gradients(c):
    return dict(g_xref=c["g_xref"], g_r_feet=c["g_r_feet"], g_yaw=c["g_yaw"], g_pos_des=c["g_pos_des"])


def tangents(c):
    return dict(d_x0=c["d_x0"], d_pos_des=c["d_pos_des"], d_cmd=c["d_cmd"],
                d_foot_lever=c["d_foot_lever"])
