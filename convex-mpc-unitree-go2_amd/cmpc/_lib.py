"""ctypes binding of the C-ABI declared in ``include/cmpc.h``.

This is the Python side of the drop-in boundary: the reference calls CasADi's conic/OSQP
plugin from Python (``centroidal_mpc.py:212-213, 98``); here Python calls ``libcmpc.so``.
The product path has no CPU fallback: if the library is missing this module raises.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

from .build import LIB

ABI_VERSION = 6
NUM_STATS = 4  # CMPC_NUM_STATS
CMPC_OK = 0


class CParams(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32),
        ("N", ctypes.c_int32),
        ("Q", ctypes.c_float * 12),
        ("R", ctypes.c_float * 12),
        ("mu", ctypes.c_float),
        ("fz_min", ctypes.c_float),
        ("eps_abs", ctypes.c_float),
        ("eps_rel", ctypes.c_float),
        ("max_iter", ctypes.c_int32),
        ("rho", ctypes.c_float),
        ("sigma", ctypes.c_float),
        ("alpha", ctypes.c_float),
        ("adaptive_rho_interval", ctypes.c_int32),
        ("polish_stable", ctypes.c_int32),
        ("polish_refine", ctypes.c_int32),
        ("polish_tol", ctypes.c_float),
        ("polish_repairs", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
        ("check_termination", ctypes.c_int32),
        ("max_batch", ctypes.c_int64),
    ]


def _io_fields(*names):
    """``size``, the arrays and values every io struct opens with, then the named fields."""
    head = ("Ad", "Bd", "gd", "x0", "xref", "contact", "mu", "fz_min")
    values = dict(face_tol=ctypes.c_float, prim_tol=ctypes.c_float, dual_tol=ctypes.c_float,
                  max_rounds=ctypes.c_int32)
    return ([("size", ctypes.c_uint32)] +
            [(n, values.get(n, ctypes.c_void_p)) for n in head + names])


class CSolveIO(ctypes.Structure):
    """cmpc_solve_io (include/cmpc.h): every argument of a solve, per-instance mu / fz_min and
    cost weights Q / R included.  ``size`` is this mirror's sizeof."""
    _fields_ = _io_fields("w_init", "y_init", "lam_init", "w_out", "y_out", "lam_out", "status",
                          "iters", "Q", "R")


class CKktIO(ctypes.Structure):
    """cmpc_kkt_io (include/cmpc.h): a batch of points to evaluate, with the per-instance values
    of CSolveIO.  ``size`` is this mirror's sizeof."""
    _fields_ = _io_fields("Q", "R", "w", "lam", "face_tol", "res")


class CGainIO(ctypes.Structure):
    """cmpc_gain_io (include/cmpc.h): a batch whose feedback gain and value function are wanted,
    with the per-instance values of CSolveIO.  ``size`` is this mirror's sizeof."""
    _fields_ = _io_fields("Q", "R", "w", "faces", "face_tol", "K", "Vx", "Vxx", "u_star",
                          "faces_out")


class CVjpIO(ctypes.Structure):
    """cmpc_vjp_io (include/cmpc.h): a batch whose gradients of a loss are wanted, given dL/dw,
    with the per-instance values of CSolveIO.  ``size`` is this mirror's sizeof."""
    _fields_ = _io_fields("Q", "R", "w", "faces", "face_tol", "gw", "g_x0", "g_xref", "g_gd", "g_Q",
                          "g_R", "g_mu", "g_fz_min", "g_Ad", "g_Bd")


class CJvpIO(ctypes.Structure):
    """cmpc_jvp_io (include/cmpc.h): a batch whose forward-mode derivative is wanted, given the
    tangents of its inputs, with the per-instance values of CSolveIO.  ``size`` is this mirror's
    sizeof."""
    _fields_ = _io_fields("Q", "R", "w", "faces", "face_tol", "d_x0", "d_xref", "d_gd", "d_Q",
                          "d_R", "d_mu", "d_fz_min", "d_Ad", "d_Bd", "dw")


class CRefineIO(ctypes.Structure):
    """cmpc_refine_io (include/cmpc.h): a batch of answers to refine and certify in float64, with
    the per-instance values of CSolveIO.  ``size`` is this mirror's sizeof."""
    _fields_ = _io_fields("Q", "R", "w", "faces", "face_tol", "max_rounds", "prim_tol", "dual_tol",
                          "info", "res", "w64", "lam_out", "faces_out", "w_out", "status")


def _dynamics_io_fields(*names):
    """``size``, cmpc_build_dynamics' four inputs and ``dt``, then the named fields."""
    head = ("mass", "inertia", "r_feet", "xref")
    return ([("size", ctypes.c_uint32)] + [(n, ctypes.c_void_p) for n in head] +
            [("dt", ctypes.c_float)] + [(n, ctypes.c_void_p) for n in names])


class CDynamicsVjpIO(ctypes.Structure):
    """cmpc_dynamics_vjp_io (include/cmpc.h): a batch of robots whose gradients through the
    dynamics builder are wanted, given dL/dAd and dL/dBd.  ``size`` is this mirror's sizeof."""
    _fields_ = _dynamics_io_fields("g_Ad", "g_Bd", "g_mass", "g_inertia", "g_r_feet", "g_yaw")


class CDynamicsJvpIO(ctypes.Structure):
    """cmpc_dynamics_jvp_io (include/cmpc.h): a batch of robots whose forward-mode derivative of
    the dynamics builder is wanted, given the tangents of its inputs.  ``size`` is this mirror's
    sizeof."""
    _fields_ = _dynamics_io_fields("d_mass", "d_inertia", "d_r_feet", "d_xref", "d_Ad", "d_Bd")


# Plan.dynamics_vjp's results (field g_<name> of cmpc_dynamics_vjp_io; yaw: the mean reference yaw)
DYNAMICS_VJP_OUTPUTS = ("mass", "inertia", "r_feet", "yaw")
# Plan.dynamics_jvp's tangents (field d_<name> of cmpc_dynamics_jvp_io) and results
DYNAMICS_JVP_TANGENTS = ("mass", "inertia", "r_feet", "xref")
DYNAMICS_JVP_OUTPUTS = ("Ad", "Bd")

def _traj_io_fields(*names):
    """``size``, cmpc_generate_traj's inputs without foot_lever and ``dt``, then the named fields."""
    head = ("x0", "pos_des", "cmd", "t_now", "gait", "hip")
    return ([("size", ctypes.c_uint32)] + [(n, ctypes.c_void_p) for n in head] +
            [("dt", ctypes.c_double)] + [(n, ctypes.c_void_p) for n in names])


class CTrajVjpIO(ctypes.Structure):
    """cmpc_traj_vjp_io (include/cmpc.h): a batch of robots whose gradients through the
    trajectory generator are wanted, given dL/dxref, dL/dr_feet, dL/dyaw_avg and the gradient in
    the desired position it leaves.  ``size`` is this mirror's sizeof."""
    _fields_ = _traj_io_fields("g_xref", "g_r_feet", "g_yaw", "g_pos_des_out", "g_x0", "g_pos_des",
                               "g_cmd", "g_foot_lever")


class CTrajJvpIO(ctypes.Structure):
    """cmpc_traj_jvp_io (include/cmpc.h): a batch of robots whose forward-mode derivative of the
    trajectory generator is wanted, given the tangents of its inputs.  ``size`` is this mirror's
    sizeof."""
    _fields_ = _traj_io_fields("d_x0", "d_pos_des", "d_cmd", "d_foot_lever", "d_xref", "d_r_feet",
                               "d_pos_des_out")


# Plan.traj_vjp's results (field g_<name> of cmpc_traj_vjp_io)
TRAJ_VJP_OUTPUTS = ("x0", "pos_des", "cmd", "foot_lever")
# Plan.traj_jvp's tangents (field d_<name> of cmpc_traj_jvp_io) and results (pos_des: the field
# d_pos_des_out, the tangent of the desired position cmpc_generate_traj leaves)
TRAJ_JVP_TANGENTS = ("x0", "pos_des", "cmd", "foot_lever")
TRAJ_JVP_OUTPUTS = ("xref", "r_feet", "pos_des")

def _srb_io_fields(*names):
    """``size``, cmpc_srb_step's arguments (``force_stride``, ``nsub`` and ``dt`` by value), then
    the named fields."""
    values = dict(force_stride=ctypes.c_int64, nsub=ctypes.c_int32, dt=ctypes.c_double)
    head = ("t_now", "gait", "mass", "inertia_body", "force", "force_stride", "hip", "x", "feet",
            "contact_state", "nsub", "dt")
    return ([("size", ctypes.c_uint32)] +
            [(n, values.get(n, ctypes.c_void_p)) for n in head + names])


class CSrbVjpIO(ctypes.Structure):
    """cmpc_srb_vjp_io (include/cmpc.h): a batch of robots whose gradients through the rigid-body
    plant are wanted, given dL/dx' and dL/dfeet'.  ``size`` is this mirror's sizeof."""
    _fields_ = _srb_io_fields("g_x_out", "g_feet_out", "g_x", "g_feet", "g_force", "g_mass",
                              "g_inertia_body")


class CSrbJvpIO(ctypes.Structure):
    """cmpc_srb_jvp_io (include/cmpc.h): a batch of robots whose forward-mode derivative of the
    rigid-body plant is wanted, given the tangents of its inputs.  ``size`` is this mirror's
    sizeof."""
    _fields_ = _srb_io_fields("d_x", "d_feet", "d_force", "d_mass", "d_inertia_body", "d_x_out",
                              "d_feet_out")


class CSrbIO(ctypes.Structure):
    """cmpc_srb_io (include/cmpc.h): cmpc_srb_step's arguments (``nsub`` and ``dt`` first), then
    the options of the force law and the wrench and the two outputs.  ``size`` is this mirror's
    sizeof."""
    _fields_ = ([("size", ctypes.c_uint32), ("nsub", ctypes.c_int32), ("dt", ctypes.c_double)] +
                [(n, ctypes.c_int64 if n == "force_stride" else ctypes.c_void_p)
                 for n in ("t_now", "gait", "mass", "inertia_body", "force", "force_stride", "hip",
                           "x", "feet", "contact_state", "K", "x_solve", "contact", "mu", "fz_min",
                           "wrench", "force_out", "fb_status")])


# Plan.srb_step's options (fields of cmpc_srb_io): inputs, then outputs
SRB_STEP_OPTIONS = ("K", "x_solve", "contact", "mu", "fz_min", "wrench", "force_out", "fb_status")
SRB_FB_HELD, SRB_FB_APPLIED, SRB_FB_CLAMPED = 0, 1, 2  # cmpc_srb_io's fb_status values

# Plan.srb_vjp's results (field g_<name> of cmpc_srb_vjp_io)
SRB_VJP_OUTPUTS = ("x", "feet", "force", "mass", "inertia_body")
# Plan.srb_jvp's tangents (field d_<name> of cmpc_srb_jvp_io) and results (field d_<name>_out)
SRB_JVP_TANGENTS = SRB_VJP_OUTPUTS
SRB_JVP_OUTPUTS = ("x", "feet")
SRB_GRAD_MAX_NSUB = 64  # CMPC_SRB_GRAD_MAX_NSUB

# cmpc_refine_io's info values below zero (CMPC_REFINE_*) and the results Plan.refine can return
REFINE_INVALID, REFINE_ROUNDS, REFINE_CYCLE, REFINE_MAX_ROUNDS = -1, -2, -3, 16
REFINE_OUTPUTS = ("info", "res", "w64", "lam", "faces")

# cmpc_gain_io's face-mask bits of a stance (step, leg): CMPC_FACE_*
FACE_FZ_MIN, FACE_FX_POS, FACE_FX_NEG, FACE_FY_POS, FACE_FY_NEG = 1, 2, 4, 8, 16
GAIN_OUTPUTS = ("K", "Vx", "Vxx", "u_star", "faces")
# Plan.vjp's results: the input each gradient belongs to (field g_<name> of cmpc_vjp_io)
VJP_OUTPUTS = ("x0", "xref", "gd", "Q", "R", "mu", "fz_min", "Ad", "Bd")
# Plan.jvp's tangents: the input each belongs to (field d_<name> of cmpc_jvp_io)
JVP_TANGENTS = VJP_OUTPUTS

KKT_COLUMNS = ("cost", "stat", "prim", "comp")  # CMPC_KKT_COST .. CMPC_KKT_COMP

NUM_BINS = 5
BIN_CAPS = (96, 128, 144, 160, 192)
# solve kernels (timing slots): 0 = bins NC 128 + 96 (two waves per SIMD), 1 = bins NC 160 + 144,
# 2 = bin NC 192 (one wave per SIMD each)
NUM_SOLVE_KERNELS = 3
KERNEL_BINS = ((1, 0), (3, 2), (4,))
KERNEL_NAMES = ("solve_group_kernel<128, 96>", "solve_group_kernel<160, 144>",
                "solve_group_kernel<192, 0>")


def _prototypes() -> dict:
    """Entry name -> (argtypes, restype) of every function include/cmpc.h declares."""
    vp, i64, rc = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    ptr = ctypes.POINTER
    table = {
        "cmpc_params_default": ([ptr(CParams)], None),
        "cmpc_plan_create": ([ptr(CParams), ptr(vp)], rc),
        "cmpc_plan_destroy": ([vp], None),
        "cmpc_solve": ([vp, i64] + [vp] * 10, rc),
        "cmpc_solve_warm": ([vp, i64] + [vp] * 13, rc),
        "cmpc_solve_ref": ([vp, i64] + [vp] * 13, rc),
        "cmpc_build_dynamics": ([vp, i64, ctypes.c_float] + [vp] * 8, rc),
        "cmpc_generate_traj": ([vp, i64, ctypes.c_double] + [vp] * 11, rc),
        "cmpc_leg_torque": ([vp, i64, vp, vp, vp, i64] + [vp] * 12 + [ctypes.c_double, vp, vp], rc),
        "cmpc_srb_step": ([vp, i64, rc, ctypes.c_double] + [vp] * 5 + [i64] + [vp] * 5, rc),
        "cmpc_plan_set_timing": ([vp, rc], rc),
        "cmpc_plan_timing_read": ([vp, ptr(ctypes.c_float), ptr(ctypes.c_int32)], rc),
        "cmpc_plan_set_team": ([vp, i64], rc),
        "cmpc_plan_team_batch": ([vp, ptr(i64)], rc),
        "cmpc_plan_set_heavy_first": ([vp, i64], rc),
        "cmpc_plan_heavy_first_batch": ([vp, ptr(i64)], rc),
        "cmpc_plan_solve_kernel": ([vp, i64, rc], ctypes.c_char_p),
        "cmpc_plan_stats": ([vp, ptr(ctypes.c_uint64), rc], rc),
        "cmpc_last_error": ([], ctypes.c_char_p),
        "cmpc_version": ([], ctypes.c_char_p),
    }
    # the struct entries: (plan, B, const io*, stream)
    for name, io in (("cmpc_solve_io_run", CSolveIO), ("cmpc_kkt_run", CKktIO),
                     ("cmpc_gain_run", CGainIO), ("cmpc_vjp_run", CVjpIO),
                     ("cmpc_refine_run", CRefineIO), ("cmpc_jvp_run", CJvpIO),
                     ("cmpc_dynamics_vjp_run", CDynamicsVjpIO),
                     ("cmpc_dynamics_jvp_run", CDynamicsJvpIO),
                     ("cmpc_traj_vjp_run", CTrajVjpIO), ("cmpc_traj_jvp_run", CTrajJvpIO),
                     ("cmpc_srb_vjp_run", CSrbVjpIO), ("cmpc_srb_jvp_run", CSrbJvpIO),
                     ("cmpc_srb_step_io_run", CSrbIO)):
        table[name] = ([vp, i64, ptr(io), vp], rc)
    return table


PROTOTYPES = _prototypes()
EXPORTS = tuple(PROTOTYPES)

_lib = None


def load(path: str | Path | None = None) -> ctypes.CDLL:
    """Load libcmpc.so (in-tree; $CMPC_LIB names a variant build, e.g. a diagnostic one) and
    declare the prototypes.  Raises if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    if path is None and os.environ.get("CMPC_LIB"):
        path = os.environ["CMPC_LIB"]
    p = Path(path) if path is not None else LIB
    if not p.exists():
        raise RuntimeError(f"cmpc: HIP library {p} not built (run __graft_entry__.build() or "
                           f"python -m cmpc.build); there is no CPU fallback")
    lib = ctypes.CDLL(str(p))
    for name, (argtypes, restype) in PROTOTYPES.items():
        if hasattr(lib, name):  # a build of other sources (A/B runs) may lack an entry: Plan._need
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, restype
    if path is None:
        _lib = lib
    return lib


def last_error(lib=None) -> str:
    lib = lib or load()
    return lib.cmpc_last_error().decode()
