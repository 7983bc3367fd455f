"""The batched MPC solve as a differentiable layer (``torch.autograd``).

``solve(plan, ...)`` is :meth:`cmpc.Plan.solve` whose ``w`` carries a gradient: the backward
pass is one :meth:`cmpc.Plan.vjp` launch (cmpc_vjp_run, include/cmpc.h) for the inputs that
require one.

The gradient is that of the fp64 optimum on the faces of the friction pyramid the returned
``w`` holds, with that face set fixed -- the function :meth:`cmpc.Plan.gain` solves -- not of the
fp32 ``w`` itself: the two differ by the solver's tolerance, and where ``w`` sits within
``face_tol`` of a face it does not hold at the true optimum (or the other way round) the
gradient is that of the neighbouring piece of the piecewise-affine law.  It does
not see a change of the face set, and it is first order only: a second backward raises.
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
        ctx.mark_non_differentiable(status, iters)
        return w, status, iters

    @staticmethod
    @once_differentiable
    def backward(ctx, gw, _gs, _gi):
        Ad, Bd, gd, x0, xref, contact, mu, fz_min, Q, R, w, status = ctx.saved_tensors
        names = _PROBLEM + (None,) + _INSTANCE           # the tensor inputs, from position 2 on
        inputs = (Ad, Bd, gd, x0, xref, contact, mu, fz_min, Q, R)
        want = [n for n, need in zip(names, ctx.needs_input_grad[2:]) if n is not None and need]
        grads = [None] * 12
        if not want:
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


def solve(plan, Ad, Bd, gd, x0, xref, contact, mu=None, fz_min=None, Q=None, R=None,
          face_tol=None):
    """:meth:`cmpc.Plan.solve` -> ``(w, status, iters)`` with ``w`` differentiable in every
    floating-point input that requires a gradient: ``Ad``, ``Bd``, ``gd``, ``x0``, ``xref`` and
    the per-robot ``mu``, ``fz_min``, ``Q``, ``R`` (None takes the plan's constant, which gets no
    gradient).  The backward pass calls :meth:`cmpc.Plan.vjp` with the saved inputs and ``w``
    for exactly the inputs that need a gradient, on the current stream, casts the float64
    results to each input's dtype, and gives a zero gradient to the rows of instances whose
    status is -10 (an invalid entry).  See the module's note on which function the gradient
    belongs to."""
    return _Solve.apply(plan, face_tol, Ad, Bd, gd, x0, xref, contact, mu, fz_min, Q, R)
