"""The batched MPC solve as a differentiable layer (``torch.autograd``).

``solve(plan, ...)`` is :meth:`cmpc.Plan.solve` whose ``w`` carries a gradient: the backward
pass is one :meth:`cmpc.Plan.vjp` launch (cmpc_vjp_run, include/cmpc.h) for the inputs that
require one, and forward-mode AD (``torch.autograd.forward_ad``) is one :meth:`cmpc.Plan.jvp`
launch (cmpc_jvp_run) for the inputs that carry a tangent.  The ``torch.func`` transforms hand a
``Function`` wrapped tensors without storage, which a native launch cannot take: ``jvp(plan, ...,
tangents)`` below is the functional form for them.

``build_dynamics(plan, ...)`` is :meth:`cmpc.Plan.build_dynamics` whose ``Ad`` and ``Bd`` carry a
gradient in the mass, the inertia, the foot levers and the reference yaw (one
:meth:`cmpc.Plan.dynamics_vjp` or :meth:`cmpc.Plan.dynamics_jvp` launch): chained
into ``solve``, a loss on the solution reaches the quantities the dynamics are built from.

``generate_traj(plan, ...)`` is :meth:`cmpc.Plan.generate_traj` whose ``xref``, ``r_feet`` and
desired position carry a gradient in the state, the desired position, the velocity command and
the current foot levers (one :meth:`cmpc.Plan.traj_vjp` or :meth:`cmpc.Plan.traj_jvp` launch,
DESIGN.md 4u): chained into ``build_dynamics`` and ``solve``, a loss on the solution reaches the
command, and the gradient in ``x0`` is the total one.

``srb_step(plan, ...)`` is :meth:`cmpc.Plan.srb_step` as a function: it steps clones and its
advanced state and feet carry a gradient in the state, the feet, the held forces, the mass and the
body inertia (one :meth:`cmpc.Plan.srb_vjp` or :meth:`cmpc.Plan.srb_jvp` launch).
``tick(plan, state, ...)`` chains the four layers into the closed loop's tick, and composing it K
times is a K-tick rollout: a loss on where the robot is after K ticks is differentiable in every
tick's command, in the initial state, and in mass and inertia (backpropagation through time), and
forward mode gives the sensitivity of the rollout.

What the gradient of a rollout sees and does not see: the face set of each tick's QP is held
(below), and so is the branch of the desired-position clamp; the contact schedule of the plant and
of the trajectory generator depends on time and gait alone, so it is exact, not held; and between
the layers the values and their gradients pass through fp32 (the dtype of ``w``, ``Ad``, ``Bd``,
``xref``, ``x``), each layer's own derivative being that of its fp64 function on those fp32
values.  A warm start does not enter: the function is the optimum on the held faces.

The gradient is that of the fp64 optimum on the faces of the friction pyramid the returned
``w`` holds, with that face set fixed -- the function :meth:`cmpc.Plan.gain` solves -- not of the
fp32 ``w`` itself: the two differ by the solver's tolerance, and where ``w`` sits within
``face_tol`` of a face it does not hold at the true optimum (or the other way round) the
gradient is that of the neighbouring piece of the piecewise-affine law.  It does
not see a change of the face set, and it is first order only: a second backward raises, and the
tangent of forward mode carries no derivative of its own.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

_PROBLEM = ("Ad", "Bd", "gd", "x0", "xref")          # positions 0..4 of the tensors passed on
_INSTANCE = ("mu", "fz_min", "Q", "R")               # positions 6..9 (5 is contact)


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, face_tol, Ad, Bd, gd, x0, xref, contact, mu, fz_min, Q, R):
        w, status, iters = plan.solve(Ad, Bd, gd, x0, xref, contact, mu=mu, fz_min=fz_min, Q=Q, R=R)
        ctx.plan, ctx.face_tol = plan, face_tol
        ctx.save_for_backward(Ad, Bd, gd, x0, xref, contact, mu, fz_min, Q, R, w, status)
        ctx.save_for_forward(Ad, Bd, gd, x0, xref, contact, mu, fz_min, Q, R, w, status)
        ctx.mark_non_differentiable(status, iters)
        ctx.set_materialize_grads(False)    # jvp: an input without a tangent arrives as None
        return w, status, iters

    @staticmethod
    @once_differentiable
    def backward(ctx, gw, _gs, _gi):
        Ad, Bd, gd, x0, xref, contact, mu, fz_min, Q, R, w, status = ctx.saved_tensors
        names = _PROBLEM + (None,) + _INSTANCE           # the tensor inputs, from position 2 on
        inputs = (Ad, Bd, gd, x0, xref, contact, mu, fz_min, Q, R)
        want = [n for n, need in zip(names, ctx.needs_input_grad[2:]) if n is not None and need]
        grads = [None] * 12
        if not want or gw is None:
            return tuple(grads)
        # (Plan.vjp launches on torch's current stream)
        res = ctx.plan.vjp(Ad, Bd, gd, x0, xref, contact,
                           gw.to(torch.float32).contiguous(), w=w, mu=mu, fz_min=fz_min, Q=Q, R=R,
                           face_tol=ctx.face_tol, want=want)
        dead = status == -10                             # an invalid instance: no gradient
        for pos, (n, t) in enumerate(zip(names, inputs)):
            if n in res:
                g = res[n].to(t.dtype)
                g[dead] = 0
                grads[2 + pos] = g
        return tuple(grads)

    @staticmethod
    def jvp(ctx, _plan, _tol, *tangents):
        Ad, Bd, gd, x0, xref, contact, mu, fz_min, Q, R, w, status = ctx.saved_tensors
        names = _PROBLEM + (None,) + _INSTANCE
        given = {n: t.detach().to(torch.float32).contiguous()
                 for n, t in zip(names, tangents) if n is not None and t is not None}
        if not given:
            return None, None, None
        # (Plan.jvp launches on torch's current stream)
        dw = ctx.plan.jvp(Ad, Bd, gd, x0, xref, contact, given, w=w, mu=mu, fz_min=fz_min, Q=Q,
                          R=R, face_tol=ctx.face_tol).to(w.dtype)
        dw[status == -10] = 0                            # an invalid instance: no tangent
        return dw, None, None


def solve(plan, Ad, Bd, gd, x0, xref, contact, mu=None, fz_min=None, Q=None, R=None,
          face_tol=None):
    """:meth:`cmpc.Plan.solve` -> ``(w, status, iters)`` with ``w`` differentiable in every
    floating-point input that requires a gradient: ``Ad``, ``Bd``, ``gd``, ``x0``, ``xref`` and
    the per-robot ``mu``, ``fz_min``, ``Q``, ``R`` (None takes the plan's constant, which gets no
    gradient).  The backward pass calls :meth:`cmpc.Plan.vjp` with the saved inputs and ``w``
    for exactly the inputs that need a gradient, on the current stream, casts the float64
    results to each input's dtype, and gives a zero gradient to the rows of instances whose
    status is -10 (an invalid entry).  Under forward-mode AD (``torch.autograd.forward_ad``)
    the tangent of ``w`` is one :meth:`cmpc.Plan.jvp` launch for exactly the
    inputs that carry a tangent, cast to ``w``'s dtype, zero in the rows of status -10.  See the
    module's note on which function the derivative belongs to."""
    return _Solve.apply(plan, face_tol, Ad, Bd, gd, x0, xref, contact, mu, fz_min, Q, R)


_DYNAMICS = ("mass", "inertia", "r_feet", "xref")    # positions 2..5 of _BuildDynamics' inputs


class _BuildDynamics(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, dt, mass, inertia, r_feet, xref):
        Ad, Bd, gd = plan.build_dynamics(mass, inertia, r_feet, xref, dt)
        ctx.plan, ctx.dt = plan, dt
        ctx.save_for_backward(mass, inertia, r_feet, xref)
        ctx.save_for_forward(mass, inertia, r_feet, xref)
        ctx.mark_non_differentiable(gd)     # a constant of dt
        ctx.set_materialize_grads(False)    # an output nothing reads arrives as None
        return Ad, Bd, gd

    @staticmethod
    @once_differentiable
    def backward(ctx, g_Ad, g_Bd, _g_gd):
        inputs = ctx.saved_tensors
        need = dict(zip(_DYNAMICS, ctx.needs_input_grad[2:]))
        want = [n if n != "xref" else "yaw" for n in _DYNAMICS if need[n]]
        grads = [None] * 6
        if not want or (g_Ad is None and g_Bd is None):
            return tuple(grads)
        f64 = torch.float64
        # (Plan.dynamics_vjp launches on torch's current stream)
        res = ctx.plan.dynamics_vjp(*inputs, ctx.dt,
                                    g_Ad=None if g_Ad is None else g_Ad.to(f64).contiguous(),
                                    g_Bd=None if g_Bd is None else g_Bd.to(f64).contiguous(),
                                    want=want)
        for pos, (n, t) in enumerate(zip(_DYNAMICS, inputs)):
            if n == "xref" and "yaw" in res:            # the mean's gradient, spread over the steps
                g = torch.zeros_like(t)
                g[:, :, 5] = (res["yaw"] / t.shape[1]).to(t.dtype)[:, None]
                grads[2 + pos] = g
            elif n in res:
                grads[2 + pos] = res[n].to(t.dtype)
        return tuple(grads)

    @staticmethod
    def jvp(ctx, _plan, _dt, *tangents):
        inputs = ctx.saved_tensors
        given = {n: t.detach().to(torch.float32).contiguous()
                 for n, t in zip(_DYNAMICS, tangents) if t is not None}
        if not given:
            return None, None, None
        # (Plan.dynamics_jvp launches on torch's current stream)
        res = ctx.plan.dynamics_jvp(*inputs, ctx.dt, given)
        return res["Ad"], res["Bd"], None


def build_dynamics(plan, mass, inertia, r_feet, xref, dt):
    """:meth:`cmpc.Plan.build_dynamics` -> ``(Ad, Bd, gd)`` with ``Ad`` and ``Bd``
    differentiable in ``mass``, ``inertia``, ``r_feet`` and ``xref`` (through the mean of its yaw
    column, which sets the rotation of the dynamics): chained into :func:`solve`, a loss on the
    solution is differentiable on the device in mass, inertia, footholds and reference yaw.
    The backward pass is one :meth:`cmpc.Plan.dynamics_vjp` launch for exactly the inputs that
    need a gradient, on the current stream: the incoming gradients are cast to float64, the
    yaw gradient is spread as ``g_yaw / N`` into column 5 of an otherwise zero ``xref`` gradient,
    and the float64 results are cast to each input's dtype.  Under forward-mode AD the tangents
    of ``Ad`` and ``Bd`` are one :meth:`cmpc.Plan.dynamics_jvp` launch for exactly the inputs
    that carry a tangent.  ``gd`` is a constant of ``dt``: it carries no gradient and its tangent
    is zero.  The derivative is that of the closed form in fp64 on the fp32 inputs, first order
    only (a second backward raises), and there is none in ``dt``.

    Composed with :func:`solve`, ``g_Ad`` and ``g_Bd`` pass through fp32 on their way here (the
    dtype of ``Ad`` and ``Bd``); the chain that stays in float64 is :meth:`cmpc.Plan.vjp` with
    ``want=("Ad", "Bd")`` -> :meth:`cmpc.Plan.dynamics_vjp`."""
    return _BuildDynamics.apply(plan, dt, mass, inertia, r_feet, xref)


_TRAJ = ("x0", "pos_des", "cmd", "foot_lever")       # positions 5..8 of _GenerateTraj's inputs


class _GenerateTraj(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, dt, t_now, gait, hip, x0, pos_des, cmd, foot_lever):
        pos_des_out = pos_des.clone()       # the caller's stays as it is: the value before the clamp
        xref, contact, r_feet = plan.generate_traj(x0, pos_des_out, cmd, t_now, gait, foot_lever,
                                                   hip, dt)
        ctx.plan, ctx.dt = plan, dt
        ctx.dtypes = (x0.dtype, pos_des.dtype, cmd.dtype, foot_lever.dtype)
        ctx.save_for_backward(x0, pos_des, cmd, t_now, gait, hip)
        ctx.save_for_forward(x0, pos_des, cmd, t_now, gait, hip)
        ctx.mark_non_differentiable(contact)
        ctx.set_materialize_grads(False)    # an output nothing reads arrives as None
        return xref, contact, r_feet, pos_des_out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_xref, _g_contact, g_r_feet, g_pos_des):
        want = [n for n, need in zip(_TRAJ, ctx.needs_input_grad[5:]) if need]
        given = dict(g_xref=g_xref, g_r_feet=g_r_feet, g_pos_des=g_pos_des)
        grads = [None] * 9
        if not want or all(g is None for g in given.values()):
            return tuple(grads)
        f64 = torch.float64
        # (Plan.traj_vjp launches on torch's current stream)
        res = ctx.plan.traj_vjp(*ctx.saved_tensors, ctx.dt, want=want,
                                **{n: None if g is None else g.to(f64).contiguous()
                                   for n, g in given.items()})
        for pos, (n, dtype) in enumerate(zip(_TRAJ, ctx.dtypes)):
            if n in res:
                grads[5 + pos] = res[n].to(dtype)
        return tuple(grads)

    @staticmethod
    def jvp(ctx, _plan, _dt, _t_now, _gait, _hip, *tangents):
        given = {n: t.detach().to(dtype).contiguous()
                 for n, t, dtype in zip(_TRAJ, tangents, ctx.dtypes) if t is not None}
        if not given:
            return None, None, None, None
        # (Plan.traj_jvp launches on torch's current stream)
        res = ctx.plan.traj_jvp(*ctx.saved_tensors, ctx.dt, given)
        return res["xref"], None, res["r_feet"], res["pos_des"]


def generate_traj(plan, x0, pos_des, cmd, t_now, gait, foot_lever, hip, dt):
    """:meth:`cmpc.Plan.generate_traj` -> ``(xref, contact, r_feet, pos_des_out)`` with ``xref``,
    ``r_feet`` and ``pos_des_out`` differentiable in ``x0``, ``pos_des``, ``cmd`` and
    ``foot_lever``: chained as ``generate_traj -> build_dynamics -> solve``, a loss on the
    solution is differentiable on the device in the velocity command, and torch sums the paths
    into ``x0`` (directly into the solve, and through the reference, the footholds and the yaw
    rotation of the dynamics), which gives the total derivative.

    The forward pass runs on a clone of ``pos_des``: the caller's tensor is not modified, the
    clamped value is returned as ``pos_des_out`` (feed it to the next tick), and the value before
    the clamp -- the one the derivative needs -- is what is saved.  ``contact`` is not
    differentiable.  The backward pass is one :meth:`cmpc.Plan.traj_vjp` launch for exactly the
    inputs that need a gradient, on the current stream: the incoming gradients are cast to
    float64 and the float64 results to each input's dtype.  Under forward-mode AD the tangents
    are one :meth:`cmpc.Plan.traj_jvp` launch for exactly the inputs that carry a tangent.  The
    contact pattern and the branch of the clamp are held fixed; the derivative is that of the
    fp64 function on the fp32 inputs, first order only (a second backward raises), and there is
    none in ``t_now``, ``gait``, ``hip`` or ``dt``.

    Composed with :func:`build_dynamics` and :func:`solve` the gradients pass through fp32 on
    their way here; the chain that stays in float64 is :meth:`cmpc.Plan.vjp` with
    ``want=("Ad", "Bd", "xref")`` -> :meth:`cmpc.Plan.dynamics_vjp` -> :meth:`cmpc.Plan.traj_vjp`
    with ``g_xref``, ``g_r_feet`` and ``g_yaw``."""
    return _GenerateTraj.apply(plan, dt, t_now, gait, hip, x0, pos_des, cmd, foot_lever)


_SRB = ("x", "feet", "force", "mass", "inertia_body")  # positions 7..11 of _SrbStep's inputs


class _SrbStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, nsub, dt, t_now, gait, hip, contact_state, x, feet, force, mass,
                inertia_body):
        x_out, feet_out, contact_out = x.clone(), feet.clone(), contact_state.clone()
        plan.srb_step(t_now, gait, mass, inertia_body, force, hip, x_out, feet_out, contact_out,
                      nsub, dt)
        ctx.plan, ctx.nsub, ctx.dt = plan, nsub, dt
        ctx.dtypes = (x.dtype, feet.dtype, force.dtype, mass.dtype, inertia_body.dtype)
        ctx.force_shape = tuple(force.shape)
        saved = (t_now, gait, mass, inertia_body, force, hip, x, feet, contact_state)
        ctx.save_for_backward(*saved)       # x, feet, contact_state: the values before the step
        ctx.save_for_forward(*saved)
        ctx.mark_non_differentiable(contact_out)
        ctx.set_materialize_grads(False)    # an output nothing reads arrives as None
        return x_out, feet_out, contact_out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_x, g_feet, _g_contact):
        want = [n for n, need in zip(_SRB, ctx.needs_input_grad[7:]) if need]
        grads = [None] * 12
        if not want or (g_x is None and g_feet is None):
            return tuple(grads)
        f64 = torch.float64
        # (Plan.srb_vjp launches on torch's current stream)
        res = ctx.plan.srb_vjp(*ctx.saved_tensors, ctx.nsub, ctx.dt,
                               g_x=None if g_x is None else g_x.to(f64).contiguous(),
                               g_feet=None if g_feet is None else g_feet.to(f64).contiguous(),
                               want=want)
        for pos, (n, dtype) in enumerate(zip(_SRB, ctx.dtypes)):
            if n in res:
                g = res[n].to(dtype)
                if n == "force" and ctx.force_shape[1] > 12:   # rows wider than U[:, 0]
                    wide = g.new_zeros(ctx.force_shape)
                    wide[:, :12] = g
                    g = wide
                grads[7 + pos] = g
        return tuple(grads)

    @staticmethod
    def jvp(ctx, _plan, _nsub, _dt, _t_now, _gait, _hip, _contact, *tangents):
        given = {n: t.detach().to(torch.float32) for n, t in zip(_SRB, tangents) if t is not None}
        if not given:
            return None, None, None
        if "force" in given:
            given["force"] = given["force"][:, :12]
        given = {n: t.contiguous() for n, t in given.items()}
        # (Plan.srb_jvp launches on torch's current stream)
        res = ctx.plan.srb_jvp(*ctx.saved_tensors, ctx.nsub, ctx.dt, given)
        return res["x"], res["feet"], None


def srb_step(plan, t_now, gait, mass, inertia_body, force, hip, x, feet, contact_state, nsub, dt):
    """:meth:`cmpc.Plan.srb_step` as a function -> ``(x', feet', contact')``: the caller's ``x``,
    ``feet`` and ``contact_state`` are not modified, the step runs on clones, and ``x'`` and
    ``feet'`` are differentiable in ``x``, ``feet``, ``force``, ``mass`` and ``inertia_body``;
    ``contact'`` is not differentiable.  ``force`` is (B, 12) fp32 or a view of such rows, e.g.
    ``w[:, 12 N:12 N + 12]`` of a solve, which carries the gradient on into :func:`solve`.

    The backward pass is one :meth:`cmpc.Plan.srb_vjp` launch for exactly the inputs that need a
    gradient, on the current stream, with the saved values from before the step: the incoming
    gradients are cast to float64 and the float64 results to each input's dtype.  Under
    forward-mode AD the tangents are one :meth:`cmpc.Plan.srb_jvp` launch for exactly the inputs
    that carry a tangent.  The contact schedule depends on ``t_now``, ``gait`` and
    ``contact_state`` alone, so the derivative is exact: that of the documented model in fp64 on
    the fp32 inputs (not of the step's fp32 arithmetic), first order only (a second backward
    raises), and there is none in ``t_now``, ``gait``, ``hip`` or ``dt``.  ``nsub`` is at most 64."""
    return _SrbStep.apply(plan, nsub, dt, t_now, gait, hip, contact_state, x, feet, force, mass,
                          inertia_body)


def tick(plan, state, cmd, gait, hip, mass, inertia_body, dt, nsub, mu=None, fz_min=None, Q=None,
         R=None):
    """One tick of :class:`cmpc.closed_loop.ClosedLoop` as a differentiable function ->
    ``(state', w, status)``.  ``state`` is a dict of ``x`` (B, 12) fp32, ``feet`` (B, 4, 3) fp32,
    ``contact_state`` (B,) uint8, ``pos_des`` (B, 3) float64 and ``t`` (B,) float64; none of its
    tensors is modified and ``state'`` holds new ones, so composing ``tick`` K times is the
    K-tick rollout.  The tick: levers ``feet - p`` and ``I_world = R I_body R'`` by torch ops,
    :func:`generate_traj` -> :func:`build_dynamics` -> :func:`solve` (cold: a warm start does not
    enter the derivative) -> :func:`srb_step` of ``nsub`` substeps of ``dt / nsub`` under
    ``w[:, 12 N:12 N + 12]``, and ``t + dt``.  ``state'["x"]``, ``["feet"]`` and ``["pos_des"]``
    and ``w`` are differentiable in ``state["x"]``, ``["feet"]``, ``["pos_des"]``, ``cmd``,
    ``mass``, ``inertia_body`` and the per-robot ``mu``, ``fz_min``, ``Q``, ``R``; see the
    module's note on what such a gradient sees."""
    from .closed_loop import rot_zyx
    N = plan.params.N
    x, feet, t = state["x"], state["feet"], state["t"]
    lever = feet - x[:, None, 0:3]
    Rm = rot_zyx(x[:, 3:6])
    RI = (Rm[:, :, :, None] * inertia_body[:, None, :, :]).sum(2)
    I_world = (RI[:, :, None, :] * Rm[:, None, :, :]).sum(3)
    xref, contact, r_feet, pos_des = generate_traj(plan, x, state["pos_des"], cmd, t, gait, lever,
                                                   hip, dt)
    Ad, Bd, gd = build_dynamics(plan, mass, I_world, r_feet, xref, dt)
    w, status, _ = solve(plan, Ad, Bd, gd, x, xref, contact, mu=mu, fz_min=fz_min, Q=Q, R=R)
    x_out, feet_out, contact_out = srb_step(plan, t, gait, mass, inertia_body,
                                            w[:, 12 * N:12 * N + 12], hip, x, feet,
                                            state["contact_state"], nsub, dt / nsub)
    return (dict(x=x_out, feet=feet_out, contact_state=contact_out, pos_des=pos_des, t=t + dt),
            w, status)


def jvp(plan, Ad, Bd, gd, x0, xref, contact, tangents, mu=None, fz_min=None, Q=None, R=None,
        face_tol=None):
    """The functional form of forward mode: :meth:`cmpc.Plan.solve` and then one
    :meth:`cmpc.Plan.jvp` launch on the faces its ``w`` holds -> ``(w, status, iters, dw)``.
    ``tangents`` is a non-empty dict from input name to a tensor of that input's shape (cast to
    fp32); ``dw`` has ``w``'s dtype and is zero in the rows of status -10, as the tangent
    ``solve`` carries under ``torch.autograd.forward_ad``."""
    w, status, iters = plan.solve(Ad, Bd, gd, x0, xref, contact, mu=mu, fz_min=fz_min, Q=Q, R=R)
    given = {n: t.detach().to(torch.float32).contiguous() for n, t in tangents.items()}
    dw = plan.jvp(Ad, Bd, gd, x0, xref, contact, given, w=w, mu=mu, fz_min=fz_min, Q=Q, R=R,
                  face_tol=face_tol).to(w.dtype)
    dw[status == -10] = 0
    return w, status, iters, dw
