"""CPU oracle (TEST INFRASTRUCTURE ONLY) -- the single-rigid-body plant behind the closed loop
(``cmpc_srb_step``, include/cmpc.h), restated from its documented model.

Per robot, with state x = [p, rpy, v, w] (w the WORLD angular velocity, rpy ZYX Euler angles,
R = R_z(yaw) R_y(pitch) R_x(roll) body -> world), held ground forces f_l and world foot positions:

  m v'           = sum_l f_l + m g                  (g = [0, 0, -9.81], stance legs only)
  I_w w' + w x I_w w = sum_l (foot_l - p) x f_l,     I_w = R I_b R'
  [roll', pitch', yaw'] = ZYX Euler rates of the world w:
      roll'  = (cy wx + sy wy) / cp,  pitch' = -sy wx + cy wy,  yaw' = wz + sp roll'

One substep of length h (semi-implicit Euler):
  1. contact: leg l is in stance iff mod(offset_l + t / period, 1) < duty at the substep's start
     time t (gait.py:21-37).  t is float64 and advances by repeated addition of h, the phase is
     evaluated in float64 in the operation order of ``stance_at`` (csrc/cmpc_traj.hip), as
     ``traj_ref.phase_mask`` does: a contact bit is a discrete quantity and has to match exactly.
  2. landing: a leg that was in swing and is now in stance is placed at z = 0 under its
     yaw-rotated hip plus half a stance of the horizontal COM velocity (Raibert, gait.py:40-74),
     p, yaw and v taken at the substep's start.
  3. accelerations from the state at the substep's start; v and w advance first, then p and rpy
     advance with the NEW v and w (the trigonometry of the Euler-rate map is the start's).

``dtype=np.float32`` runs the same formulas with every state operation rounded to float32 (time
and gait phase stay float64, as in the kernel).  It is not a second reference: the gap between
the two modes on a given input is the size of float32 rounding noise in this computation, and
the tests scale their tolerances by it.

``model`` selects the formulas: :class:`Plant` is the documented model.  tests/test_srb.py
subclasses it with deliberate mistakes to show that its inputs tell them apart.

Only tests/ may import this file; the product path never does.

Batched layouts (the C-ABI's):
  x (B,12); feet (B,4,3); contact_state (B,) uint8, bit l = leg l in stance; t_now (B,) float64;
  gait (B,6) float64 = [period, duty, offset FL, FR, RL, RR]; mass (B,); inertia_body (B,3,3);
  force (B,12) = U[:, 0], leg-major; hip (4,3) body frame
  -> x' (B,12), feet' (B,4,3), contact_state' (B,) uint8.
"""
from __future__ import annotations

import numpy as np

GRAVITY = 9.81


class Plant:
    """The documented model, one overridable piece per modelling decision."""

    @staticmethod
    def rotation(rpy):
        """(B,3) -> (B,3,3) R = R_z R_y R_x, in rpy's dtype."""
        r, p, y = rpy[:, 0], rpy[:, 1], rpy[:, 2]
        cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
        R = np.empty((len(rpy), 3, 3), rpy.dtype)
        R[:, 0, 0] = cy * cp
        R[:, 0, 1] = cy * sp * sr - sy * cr
        R[:, 0, 2] = cy * sp * cr + sy * sr
        R[:, 1, 0] = sy * cp
        R[:, 1, 1] = sy * sp * sr + cy * cr
        R[:, 1, 2] = sy * sp * cr - cy * sr
        R[:, 2, 0] = -sp
        R[:, 2, 1] = cp * sr
        R[:, 2, 2] = cp * cr
        return R

    @staticmethod
    def inertia_world(R, Ib):
        return R @ Ib @ np.swapaxes(R, 1, 2)

    @staticmethod
    def gyroscopic(w, Iw):
        """w x I_w w."""
        return np.cross(w, np.einsum('bij,bj->bi', Iw, w))

    @staticmethod
    def euler_rates(rpy, w):
        """ZYX Euler-angle rates of the world angular velocity w."""
        p, y = rpy[:, 1], rpy[:, 2]
        cp, sp, cy, sy = np.cos(p), np.sin(p), np.cos(y), np.sin(y)
        rd = (cy * w[:, 0] + sy * w[:, 1]) / cp
        pd = -sy * w[:, 0] + cy * w[:, 1]
        yd = w[:, 2] + sp * rd
        return np.stack([rd, pd, yd], 1)

    @staticmethod
    def contact_time(t, h):
        """The time at which a substep starting at t reads the gait."""
        return t

    @staticmethod
    def touchdown(p, yaw, v, hip_l, t_stance):
        """(B,3) landing position of the leg with body-frame hip offset hip_l."""
        cy, sy = np.cos(yaw), np.sin(yaw)
        half = t_stance / t_stance.dtype.type(2)
        return np.stack([p[:, 0] + (cy * hip_l[0] - sy * hip_l[1]) + v[:, 0] * half,
                         p[:, 1] + (sy * hip_l[0] + cy * hip_l[1]) + v[:, 1] * half,
                         np.zeros_like(yaw)], 1)

    @staticmethod
    def advance_position(p, v_old, v_new, h):
        return p + h * v_new


def stance_mask(t, period, duty, offsets):
    """(B,) float64 times -> (B,4) bool, ``stance_at``'s operation order."""
    ph = np.mod(offsets + (t / period)[:, None], 1.0)
    return ph < duty[:, None]


def srb_step(x, feet, contact_state, t_now, gait, mass, inertia_body, force, hip, h, nsub,
             dtype=np.float64, model=Plant):
    """``nsub`` substeps of length ``h`` from ``t_now``; returns (x, feet, contact_state)."""
    ft = np.dtype(dtype).type
    x = np.array(x, dtype=ft)
    B = x.shape[0]
    p, rpy, v, w = x[:, 0:3].copy(), x[:, 3:6].copy(), x[:, 6:9].copy(), x[:, 9:12].copy()
    feet = np.array(feet, dtype=ft).reshape(B, 4, 3)
    f = np.asarray(force, dtype=ft).reshape(B, 4, 3)
    m = np.asarray(mass, dtype=ft).reshape(B)
    Ib = np.asarray(inertia_body, dtype=ft).reshape(B, 3, 3)
    hip = np.asarray(hip, dtype=ft).reshape(4, 3)
    gait = np.asarray(gait, np.float64)
    period, duty, offs = gait[:, 0], gait[:, 1], gait[:, 2:6]
    t_stance = (duty * period).astype(ft)
    t = np.array(t_now, np.float64).reshape(B)
    hs = ft(h)
    g = np.array([0, 0, -GRAVITY], dtype=ft)
    bits = np.asarray(contact_state, np.uint8).reshape(B)
    stance = ((bits[:, None] >> np.arange(4, dtype=np.uint8)) & 1).astype(bool)
    for _ in range(int(nsub)):
        now = stance_mask(model.contact_time(t, float(h)), period, duty, offs)
        for leg in range(4):
            land = now[:, leg] & ~stance[:, leg]
            if land.any():
                td = model.touchdown(p, rpy[:, 2], v, hip[leg], t_stance)
                feet[land, leg] = td[land]
        stance = now
        Iw = model.inertia_world(model.rotation(rpy), Ib)
        fs = f * stance[:, :, None].astype(ft)
        lever = feet - p[:, None, :]
        torque = np.cross(lever, fs).sum(1)
        v_new = v + hs * (fs.sum(1) / m[:, None] + g)
        wd = np.linalg.solve(Iw, (torque - model.gyroscopic(w, Iw))[:, :, None])[:, :, 0]
        w = w + hs * wd
        p = model.advance_position(p, v, v_new, hs)
        v = v_new
        rpy = rpy + hs * model.euler_rates(rpy, w)
        t = t + float(h)
    out = (stance.astype(np.uint8) << np.arange(4, dtype=np.uint8)).sum(1).astype(np.uint8)
    return np.concatenate([p, rpy, v, w], 1), feet, out
