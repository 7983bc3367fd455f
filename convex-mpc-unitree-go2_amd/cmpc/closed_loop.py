"""Batched closed loop on the device: many robots, one MPC tick per call, everything resident.

The reference's loop (test_MPC.py:160-236) runs per robot on the CPU: every STEPS_PER_MPC leg
ticks it calls ``traj.generate_traj`` and ``mpc.solve_QP`` (warm-started) and holds U[:, 0]
until the next MPC tick; MuJoCo integrates the robot.  Here one call of :meth:`ClosedLoop.tick`
does that for B robots with no host round trip:

  cmpc_generate_traj -> cmpc_build_dynamics -> cmpc_solve_io_run -> cmpc_srb_step (nsub substeps)

MuJoCo and the Go2 model are absent from this image, so the plant is ``cmpc_srb_step``'s
single-rigid-body stand-in (include/cmpc.h) and the robot quantities Pinocchio would supply are
the synthetic ones of :mod:`cmpc.synth` (mass, body inertia, hip offsets).  :meth:`capture`
records one tick as a HIP graph (``torch.cuda.CUDAGraph``) so that a tick is one graph launch.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import synth
from .solver import Plan, SolverParams


def rot_zyx(rpy: torch.Tensor) -> torch.Tensor:
    """(B,3) roll, pitch, yaw -> (B,3,3) R_z R_y R_x (the base rotation whose ZYX angles are the
    MPC state's rpy, go2_robot_data.py:211-216)."""
    r, p, y = rpy.unbind(-1)
    cr, sr, cp, sp, cy, sy = r.cos(), r.sin(), p.cos(), p.sin(), y.cos(), y.sin()
    return torch.stack([cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr,
                        sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr,
                        -sp, cp * sr, cp * cr], -1).reshape(-1, 3, 3)


class ClosedLoop:
    """B robots walking under batched MPC (test_MPC.py's loop shape, MPC_DT = gait period / N).

    ``mu`` / ``fz_min``: per-robot friction coefficient and stance normal-force floor, (B,)
    values (None: the plan's constants).  The loop keeps them as the device tensors ``self.mu``
    / ``self.fz_min`` and passes them to every solve by pointer: writing new values into them in
    place (``loop.mu.copy_(...)``, a terrain estimator's output) takes effect at the next tick,
    a replay of the captured graph included.  They bound the forces the MPC plans; the
    single-rigid-body plant has no friction model and applies the planned forces as they are.

    ``Q`` / ``R``: per-robot cost weights, (B, 12) or (12,) values (None: the plan's constants),
    kept the same way as the device tensors ``self.Q`` / ``self.R``: a supervisor that writes a
    robot's row in place re-weights that robot from the next tick on.

    ``report=True``: every tick also evaluates the returned forces on the device (``Plan.kkt``
    with recovered multipliers, the loop's ``mu`` / ``fz_min`` / ``Q`` / ``R``) into ``self.kkt``,
    a (B, 4) float64 tensor with the columns ``cmpc.KKT_COLUMNS``: a per-robot health signal
    besides ``status``.  ``self.x_solve`` holds the state the tick solved from (the plant
    overwrites ``x``).  Both run on the tick's stream, so a captured graph carries them.

    ``gain=True``: every tick also evaluates the feedback gain of the returned forces
    (``Plan.gain`` on the faces ``w`` holds) into ``self.K0``, a (B, 12, 12) float64 tensor with
    ``K0[b] = d U[:, 0] / d x0``: between two MPC ticks ``U[:, 0] + K0 (x - x_solve)`` is the
    first-order correction of the held forces.  It runs on the tick's stream too and keeps
    ``self.x_solve`` as ``report`` does.

    ``feedback=True`` (implies ``gain``): the plant applies that correction at every substep
    (``Plan.srb_step`` with ``K0``, ``x_solve``, the contact table and the loop's ``mu`` /
    ``fz_min``), each leg the MPC planned in stance kept inside its friction pyramid;
    ``self.fb_status`` (B,) uint8 says per robot whether the law was held (0: ``K0`` not finite,
    ``mu`` / ``fz_min`` invalid), applied (1) or applied and clamped (2).

    ``push=True``: ``self.wrench``, a (B, 6) fp32 tensor of zeros, is the external wrench on every
    robot (world force at the COM, world torque about it).  Written in place, it takes effect at
    the next tick, a replay of the captured graph included, and is held until rewritten."""

    def __init__(self, B: int, plan: Optional[Plan] = None, gait_hz: float = synth.GAIT_HZ,
                 duty: float = synth.GAIT_DUTY, offsets=synth.TROT_OFFSETS, nsub: int = 20,
                 seed: int = 0, device="cuda", shift_warm: bool = True, mu=None, fz_min=None,
                 Q=None, R=None, report: bool = False, gain: bool = False,
                 feedback: bool = False, push: bool = False):
        self.plan = plan or Plan(SolverParams(max_batch=B))
        self.B, self.N = B, self.plan.params.N
        dev = torch.device(device)
        self.dev = dev
        self.period = 1.0 / gait_hz
        self.dt = self.period / self.N                    # test_MPC.py:67-68
        self.nsub = nsub                                  # leg ticks per MPC tick (:69)
        f32, f64 = torch.float32, torch.float64
        rng = np.random.default_rng(seed)
        yaw0 = rng.uniform(-np.pi, np.pi, B)
        x = np.zeros((B, 12))
        x[:, 0:2] = rng.uniform(-1, 1, (B, 2))
        x[:, 2] = synth.Z_DES
        x[:, 5] = yaw0
        self.x = torch.as_tensor(x, dtype=f32, device=dev).contiguous()
        self.pos_des = self.x[:, 0:3].to(f64).clone()     # ComTraj.__init__ (com_trajectory.py:12-13)
        self.t = torch.zeros(B, dtype=f64, device=dev)
        self.gait = torch.tensor([self.period, duty, *offsets], dtype=f64,
                                 device=dev).repeat(B, 1).contiguous()
        self.hip = torch.as_tensor(synth.HIP_OFFSETS, dtype=f32, device=dev).contiguous()
        self.mass = torch.full((B,), synth.MASS, dtype=f32, device=dev)
        self.I_body = torch.as_tensor(synth.INERTIA_BODY, dtype=f32, device=dev).repeat(B, 1, 1).contiguous()
        c, s = np.cos(yaw0), np.sin(yaw0)
        hipw = np.stack([np.stack([x[:, 0] + c * hx - s * hy, x[:, 1] + s * hx + c * hy,
                                   np.zeros(B)], -1) for hx, hy in synth.HIP_XY], 1)
        self.feet = torch.as_tensor(hipw, dtype=f32, device=dev).contiguous()
        self.contact = torch.full((B,), 0xF, dtype=torch.uint8, device=dev)
        N = self.N
        self.cmd = torch.zeros((B, 4), dtype=f32, device=dev)
        self.cmd[:, 2] = synth.Z_DES
        self.xref = torch.empty((B, N, 12), dtype=f32, device=dev)
        self.ct = torch.empty((B, 4, N), dtype=torch.uint8, device=dev)
        self.rf = torch.empty((B, N, 4, 3), dtype=f32, device=dev)
        self.Ad = torch.empty((B, 12, 12), dtype=f32, device=dev)
        self.Bd = torch.empty((B, N, 12, 12), dtype=f32, device=dev)
        self.gd = torch.empty((B, 12), dtype=f32, device=dev)
        self.w = torch.zeros((B, 24 * N), dtype=f32, device=dev)
        self.y = torch.zeros((B, 12 * N), dtype=f32, device=dev)
        self.status = torch.empty((B,), dtype=torch.int32, device=dev)
        self.iters = torch.empty((B,), dtype=torch.int32, device=dev)
        self.lever = torch.empty((B, 4, 3), dtype=f32, device=dev)
        self.I_world = torch.empty((B, 3, 3), dtype=f32, device=dev)
        self.w_init = torch.zeros_like(self.w)
        self.y_init = torch.zeros_like(self.y)
        self.mu, self.fz_min = (
            None if v is None else
            torch.as_tensor(v, dtype=f32).expand(B).contiguous().to(dev, copy=True)
            for v in (mu, fz_min))
        self.Q, self.R = (
            None if v is None else
            torch.as_tensor(v, dtype=f32).expand(B, 12).contiguous().to(dev, copy=True)
            for v in (Q, R))
        self.report = bool(report)
        self.feedback = bool(feedback)
        self.gain = bool(gain) or self.feedback
        if self.report or self.gain:
            self.x_solve = torch.empty_like(self.x)
        if self.report:
            self.kkt = torch.empty((B, 4), dtype=f64, device=dev)
        if self.gain:
            self.K0 = torch.empty((B, 12, 12), dtype=f64, device=dev)
        # the plant's options (Plan.srb_step): none by default, so the tick is cmpc_srb_step's
        self.plant = {}
        if self.feedback:
            self.fb_status = torch.zeros((B,), dtype=torch.uint8, device=dev)
            self.plant.update(K=self.K0, x_solve=self.x_solve, contact=self.ct, mu=self.mu,
                              fz_min=self.fz_min, fb_status=self.fb_status)
        if push:
            self.wrench = torch.zeros((B, 6), dtype=f32, device=dev)
            self.plant.update(wrench=self.wrench)
        self.shift_warm = shift_warm
        self.warm = False
        self.graph = None

    def set_command(self, cmd):
        """(B,4) [vx_body, vy_body, z_des, yaw_rate] (test_MPC.py get_body_cmd)."""
        self.cmd.copy_(torch.as_tensor(cmd, dtype=torch.float32, device=self.dev))

    def _tick(self, stream, warm: bool):
        p, N, B = self.plan, self.N, self.B
        # what generate_traj reads off the robot: levers COM -> foot, I_com in the world frame
        torch.sub(self.feet, self.x[:, None, 0:3], out=self.lever)
        R = rot_zyx(self.x[:, 3:6])
        # R I_body R' as broadcast products + size-3 sums: batched 3x3 GEMMs go to the BLAS
        # library, two launches of ~0.57 ms each at 65,536 robots (rocprofv3, tools/loop_graph.py)
        RI = (R[:, :, :, None] * self.I_body[:, None, :, :]).sum(2)
        torch.sum(RI[:, :, None, :] * R[:, None, :, :], 3, out=self.I_world)
        p.generate_traj(self.x, self.pos_des, self.cmd, self.t, self.gait, self.lever, self.hip,
                        self.dt, out=(self.xref, self.ct, self.rf), stream=stream)
        p.build_dynamics(self.mass, self.I_world, self.rf, self.xref, self.dt,
                         out=(self.Ad, self.Bd, self.gd), stream=stream)
        if warm and self.shift_warm:
            # the previous tick's plan, moved one MPC step forward (its step k+1 is this tick's k;
            # the last step repeats): the contact schedule shifts the same way, so the warm face
            # set lines up with this tick's QP
            U, Ui = self.w[:, 12 * N:].view(B, N, 12), self.w_init[:, 12 * N:].view(B, N, 12)
            Ui[:, :-1].copy_(U[:, 1:]); Ui[:, -1].copy_(U[:, -1])
            Y, Yi = self.y.view(B, N, 12), self.y_init.view(B, N, 12)
            Yi[:, :-1].copy_(Y[:, 1:]); Yi[:, -1].copy_(Y[:, -1])
            kw = dict(w_init=self.w_init, y_init=self.y_init)
        else:
            kw = dict(w_init=self.w, y_init=self.y) if warm else {}
        if self.report or self.gain:
            self.x_solve.copy_(self.x)
        p.solve(self.Ad, self.Bd, self.gd, self.x, self.xref, self.ct,
                out=(self.w, self.status, self.iters), stream=stream, y_out=self.y,
                mu=self.mu, fz_min=self.fz_min, Q=self.Q, R=self.R, **kw)
        if self.report:
            p.kkt(self.Ad, self.Bd, self.gd, self.x_solve, self.xref, self.ct, self.w,
                  mu=self.mu, fz_min=self.fz_min, Q=self.Q, R=self.R, out=self.kkt, stream=stream)
        if self.gain:
            p.gain(self.Ad, self.Bd, self.gd, self.x_solve, self.xref, self.ct, w=self.w,
                   mu=self.mu, fz_min=self.fz_min, Q=self.Q, R=self.R, out=dict(K=self.K0),
                   stream=stream)
        # the plant reads U[:, 0] off the rows of w (test_MPC.py:196)
        p.srb_step(self.t, self.gait, self.mass, self.I_body, self.w[:, 12 * N:], self.hip, self.x,
                   self.feet, self.contact, self.nsub, self.dt / self.nsub, stream=stream,
                   **self.plant)
        self.t.add_(self.dt)

    def tick(self):
        """One MPC tick for every robot (graph replay once :meth:`capture` has run)."""
        if self.graph is not None:
            self.graph.replay()
            return
        self._tick(torch.cuda.current_stream(self.dev), self.warm)
        self.warm = True

    def capture(self):
        """Record one warm tick as a HIP graph (after at least one eager tick)."""
        if not self.warm:
            self.tick()
        s = torch.cuda.Stream(self.dev)
        s.wait_stream(torch.cuda.current_stream(self.dev))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            self._tick(s, True)
        torch.cuda.current_stream(self.dev).wait_stream(s)
        self.graph = g
        # capture recorded the work without running it: nothing to undo
