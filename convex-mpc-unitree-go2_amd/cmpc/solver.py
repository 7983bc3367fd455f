"""Batched solver on device tensors: the C-ABI wrapped for PyTorch-ROCm buffers.

``Plan`` mirrors what ``CentroidalMPC.__init__`` builds once (``centroidal_mpc.py:41-67``:
constants, sparsity, solver object); ``Plan.solve`` is the batched equivalent of
``solve_QP``'s update + solve (``centroidal_mpc.py:69-120``).  PyTorch is used only for device
memory and streams.
"""
from __future__ import annotations

import ctypes
import functools
from dataclasses import dataclass, field, fields
from typing import Optional

import torch

from . import _lib

STATUS_STRINGS = {1: "solved", 2: "solved inaccurate", -2: "maximum iterations reached",
                  -10: "unsolved"}
KKT_COLUMNS = _lib.KKT_COLUMNS   # the columns of Plan.kkt's result


@dataclass
class SolverParams:
    """cmpc_params (include/cmpc.h).  Defaults = the reference's constants
    (centroidal_mpc.py:12-38, :127) plus this solver's ADMM/polish settings."""
    N: int = 16
    Q: tuple = (1, 1, 50, 10, 20, 1, 2, 2, 1, 1, 1, 1)
    R: tuple = (1e-5,) * 12
    mu: float = 0.8
    fz_min: float = 10.0
    eps_abs: float = 1e-4
    eps_rel: float = 1e-4
    max_iter: int = 1000
    rho: float = 1e-4
    sigma: float = 1e-6
    alpha: float = 1.6
    adaptive_rho_interval: int = 25
    polish_stable: int = 3
    polish_refine: int = 2
    polish_tol: float = 1e-5
    polish_repairs: int = 6
    check_termination: int = 1   # OPTS check_termination (reference: 10; include/cmpc.h)
    max_batch: int = 65536

    def to_c(self) -> _lib.CParams:
        c = _lib.CParams()
        c.abi_version = _lib.ABI_VERSION
        for f in fields(self):
            val = getattr(self, f.name)
            if f.name in ("Q", "R"):
                if len(val) != 12:
                    raise ValueError(f"{f.name} must have 12 entries")
                setattr(c, f.name, (ctypes.c_float * 12)(*[float(v) for v in val]))
            else:
                setattr(c, f.name, val)
        return c


class CmpcError(RuntimeError):
    pass


def _check(lib, rc: int, what: str):
    if rc != _lib.CMPC_OK:
        raise CmpcError(f"{what} failed ({rc}): {_lib.last_error(lib)}")


def _stream_ptr(stream, device) -> ctypes.c_void_p:
    """``stream`` (None: torch's current stream on ``device``) as the C-ABI's ``void*``."""
    if stream is None:
        stream = torch.cuda.current_stream(device)
    return ctypes.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else stream)


# The specs: name -> (dtype, shape) of the tensors of an entry.  They depend on the sizes alone, so
# a loop that calls with the same sizes every tick builds them once; callers do not modify them.
_spec = functools.lru_cache(maxsize=32)


@_spec
def _problem_spec(B, N) -> dict:
    """The six arrays of a batch of B problems and the optional per-instance values."""
    f32 = torch.float32
    return dict(Ad=(f32, (B, 12, 12)), Bd=(f32, (B, N, 12, 12)), gd=(f32, (B, 12)),
                x0=(f32, (B, 12)), xref=(f32, (B, N, 12)), contact=(torch.uint8, (B, 4, N)),
                mu=(f32, (B,)), fz_min=(f32, (B,)), Q=(f32, (B, 12)), R=(f32, (B, 12)))


@_spec
def _solve_spec(B, N) -> dict:
    """Every tensor of a solve: the problem, the warm starts and dual outputs and the three
    results."""
    f32, i32 = torch.float32, torch.int32
    nw, ny, nl = 24 * N, 12 * N, 52 * N
    return dict(_problem_spec(B, N), w_init=(f32, (B, nw)), y_init=(f32, (B, ny)),
                lam_init=(f32, (B, nl)), y_out=(f32, (B, ny)), lam_out=(f32, (B, nl)),
                w=(f32, (B, nw)), status=(i32, (B,)), iters=(i32, (B,)))


@_spec
def _eval_spec(B, N) -> dict:
    """Every input of the evaluation entries (kkt, gain, vjp, refine): the problem, the points,
    their multipliers or held faces, dL/dw, and refine's in-place w_out / status."""
    f32 = torch.float32
    return dict(_problem_spec(B, N), w=(f32, (B, 24 * N)), lam=(f32, (B, 52 * N)),
                faces=(torch.uint8, (B, N, 4)), gw=(f32, (B, 24 * N)), w_out=(f32, (B, 24 * N)),
                status=(torch.int32, (B,)))


@_spec
def _dynamics_spec(B, N) -> tuple:
    """(inputs, results) of cmpc_build_dynamics."""
    f32, p = torch.float32, _problem_spec(B, N)
    return (dict(mass=(f32, (B,)), inertia=(f32, (B, 3, 3)), r_feet=(f32, (B, N, 4, 3)),
                 xref=p["xref"]), {k: p[k] for k in ("Ad", "Bd", "gd")})


@_spec
def _dynamics_grad_spec(B, N) -> tuple:
    """(gradients in, gradients out, tangents in, tangents out) of cmpc_dynamics_vjp_run and
    cmpc_dynamics_jvp_run; the two results are name -> (io field, dtype, shape)."""
    f32, f64 = torch.float32, torch.float64
    inputs, outputs = _dynamics_spec(B, N)
    return (dict(g_Ad=(f64, (B, 12, 12)), g_Bd=(f64, (B, N, 12, 12))),
            dict(mass=("g_mass", f64, (B,)), inertia=("g_inertia", f64, (B, 3, 3)),
                 r_feet=("g_r_feet", f64, (B, N, 4, 3)), yaw=("g_yaw", f64, (B,))),
            {"d_" + n: s for n, s in inputs.items()},
            {n: ("d_" + n, *outputs[n]) for n in _lib.DYNAMICS_JVP_OUTPUTS})


@_spec
def _traj_spec(B, N) -> tuple:
    """(inputs, results) of cmpc_generate_traj."""
    f32, f64, p = torch.float32, torch.float64, _problem_spec(B, N)
    return (dict(x0=p["x0"], pos_des=(f64, (B, 3)), cmd=(f32, (B, 4)), t_now=(f64, (B,)),
                 gait=(f64, (B, 6)), foot_lever=(f32, (B, 4, 3)), hip=(f32, (4, 3))),
            dict(xref=p["xref"], contact=p["contact"], r_feet=(f32, (B, N, 4, 3))))


@_spec
def _traj_grad_spec(B, N) -> tuple:
    """(inputs, gradients in, gradients out, tangents in, tangents out) of cmpc_traj_vjp_run and
    cmpc_traj_jvp_run; the two results are name -> (io field, dtype, shape)."""
    f32, f64 = torch.float32, torch.float64
    inputs, outputs = _traj_spec(B, N)
    moving = {n: inputs[n] for n in _lib.TRAJ_VJP_OUTPUTS}
    return ({n: s for n, s in inputs.items() if n != "foot_lever"},
            dict(g_xref=(f64, (B, N, 12)), g_r_feet=(f64, (B, N, 4, 3)), g_yaw=(f64, (B,)),
                 g_pos_des_out=(f64, (B, 3))),
            {n: ("g_" + n, f64, shape) for n, (_, shape) in moving.items()},
            {"d_" + n: s for n, s in moving.items()},
            dict(xref=("d_xref", *outputs["xref"]), r_feet=("d_r_feet", *outputs["r_feet"]),
                 pos_des=("d_pos_des_out", f64, (B, 3))))


@_spec
def _leg_spec(B) -> tuple:
    """(inputs, results) of cmpc_leg_torque, ``force`` apart (_force_rows)."""
    f64 = torch.float64
    return (dict(t=(f64, (B,)), gait=(f64, (B, 6)), J_foot=(f64, (B, 4, 3, 3)),
                 J_full=(f64, (B, 4, 3, 18)), M=(f64, (B, 18, 18)), C=(f64, (B, 18, 18)),
                 g=(f64, (B, 18)), dq=(f64, (B, 18)), Jdot_dq=(f64, (B, 4, 3)),
                 foot_pos=(f64, (B, 4, 3)), foot_vel=(f64, (B, 4, 3)), body=(f64, (B, 16)),
                 hip=(f64, (4, 3)), state=(f64, (B, 4, 8))), dict(tau=(f64, (B, 12))))


@_spec
def _srb_spec(B) -> tuple:
    """(inputs, results) of cmpc_srb_step, ``force`` apart: x, feet and contact_state are
    updated in place and there is no result."""
    f32, f64 = torch.float32, torch.float64
    return (dict(t_now=(f64, (B,)), gait=(f64, (B, 6)), mass=(f32, (B,)),
                 inertia_body=(f32, (B, 3, 3)), hip=(f32, (4, 3)), x=(f32, (B, 12)),
                 feet=(f32, (B, 4, 3)), contact_state=(torch.uint8, (B,))), {})


@_spec
def _srb_io_spec(B, N) -> dict:
    """The options of cmpc_srb_step_io_run (cmpc_srb_io's fields after contact_state)."""
    f32, u8 = torch.float32, torch.uint8
    return dict(K=(torch.float64, (B, 12, 12)), x_solve=(f32, (B, 12)), contact=(u8, (B, 4, N)),
                mu=(f32, (B,)), fz_min=(f32, (B,)), wrench=(f32, (B, 6)),
                force_out=(f32, (B, 12)), fb_status=(u8, (B,)))


@_spec
def _srb_grad_spec(B) -> tuple:
    """(inputs, gradients in, gradients out, tangents in, tangents out) of cmpc_srb_vjp_run and
    cmpc_srb_jvp_run, ``force`` apart (_force_rows); the two results are name -> (io field, dtype,
    shape).  ``force``'s gradient and tangent are packed (B, 12)."""
    f32, f64 = torch.float32, torch.float64
    inputs, _ = _srb_spec(B)
    moving = dict(x=(B, 12), feet=(B, 4, 3), force=(B, 12), mass=(B,), inertia_body=(B, 3, 3))
    return (inputs,
            dict(g_x_out=(f64, (B, 12)), g_feet_out=(f64, (B, 4, 3))),
            {n: ("g_" + n, f64, moving[n]) for n in _lib.SRB_VJP_OUTPUTS},
            {"d_" + n: (f32, moving[n]) for n in _lib.SRB_JVP_TANGENTS},
            {n: ("d_" + n + "_out", f32, moving[n]) for n in _lib.SRB_JVP_OUTPUTS})


def _problem(Ad, Bd, gd, x0, xref, contact, **more) -> dict:
    """name -> tensor of the six problem arrays and what else an entry requires."""
    return dict(Ad=Ad, Bd=Bd, gd=gd, x0=x0, xref=xref, contact=contact, **more)


def _force_rows(force, B, device) -> torch.Tensor:
    """The one strided argument of the pipeline entries: forces as (B, 12) fp32 or a (B, >=12)
    fp32 view whose rows start at U[:, 0] (e.g. w[:, 12N:]); its row stride goes with it."""
    if (not isinstance(force, torch.Tensor) or force.device != device or
            force.dtype != torch.float32 or force.dim() != 2 or force.shape[0] != B or
            force.shape[1] < 12 or force.stride(1) != 1):
        raise ValueError("force must be a (B, >=12) fp32 tensor on the plan's device with unit "
                         "column stride")
    return force


class Plan:
    """Owns a cmpc_plan (device workspace for up to params.max_batch instances)."""

    def __init__(self, params: Optional[SolverParams] = None, device=None):
        self.params = params or SolverParams()
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise CmpcError("cmpc: no ROCm device available (the solver has no CPU fallback)")
        dv = torch.device("cuda") if device is None else torch.device(device)
        if dv.type != "cuda":
            raise ValueError(f"cmpc: plan device must be a ROCm (cuda) device, got {dv}")
        self.device = torch.device("cuda", torch.cuda.current_device() if dv.index is None
                                   else dv.index)
        with torch.cuda.device(self.device):
            h = ctypes.c_void_p()
            cp = self.params.to_c()
            d = _lib.CParams()
            self.lib.cmpc_params_default(ctypes.byref(d))
            if d.abi_version != _lib.ABI_VERSION:
                raise CmpcError(f"cmpc: library ABI {d.abi_version}, this binding is ABI "
                                f"{_lib.ABI_VERSION}")
            _check(self.lib, self.lib.cmpc_plan_create(ctypes.byref(cp), ctypes.byref(h)),
                   "cmpc_plan_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.cmpc_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _address(self, t, name: str, dtype, shape) -> int:
        """The address of tensor ``t`` once it is what the spec says: of that dtype and shape,
        contiguous, and on the plan's device (where its workspace and streams live)."""
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.device != self.device:
            if t.device.type != "cuda":
                raise ValueError(f"{name} must be a device (cuda/ROCm) tensor")
            raise ValueError(f"cmpc: {name} is on {t.device} but the plan was created on "
                             f"{self.device}")
        if t.dtype != dtype:
            raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
        if t.shape != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        return t.data_ptr()

    def _fill_io(self, io, spec: dict, required: dict, optional: dict, fields: dict = {}):
        """Check required's and optional's name -> tensor against spec's name -> (dtype, shape), in
        their order, and point io's fields of those names (``fields``: name -> field where the
        two differ) at them; an optional tensor that is None is skipped (NULL)."""
        for name, t in required.items():
            setattr(io, fields.get(name, name), self._address(t, name, *spec[name]))
        for name, t in optional.items():
            if t is not None:
                setattr(io, name, self._address(t, name, *spec[name]))

    def _need(self, entry: str, method: str):
        """An evaluation entry that a library built from older sources does not have."""
        if not hasattr(self.lib, entry):
            raise CmpcError(f"cmpc: this libcmpc.so has no {entry}: Plan.{method} needs a library "
                            "built from sources that declare it")

    def _results(self, io, spec: dict, want, always, out, device) -> dict:
        """The results ``always`` + ``want`` of an evaluation entry, taken from ``out`` or
        allocated on ``device`` and checked against spec's name -> (io field, dtype, shape), with
        io's fields pointed at them: the dict the entry returns."""
        out = dict(out or {})
        res = {}
        for name in tuple(always) + tuple(n for n in want if n not in always):
            field, dtype, shape = spec[name]
            t = out.get(name)
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=device)
            setattr(io, field, self._address(t, name, dtype, shape))
            res[name] = t
        return res

    def _run_io(self, entry: str, io, B: int, stream):
        """Call a struct entry on the plan's device; a failure raises with the library's message."""
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, entry)(self._h, B, ctypes.byref(io),
                                          _stream_ptr(stream, self.device))
        _check(self.lib, rc, entry)

    def _pipeline(self, entry, spec, tensors, out, stream, args) -> tuple:
        """A pipeline entry's wrapper.  ``spec`` is (inputs, results), each name -> (dtype, shape):
        check ``tensors`` as the inputs; take the results from the tuple ``out`` or allocate them,
        and check them the same way; call ``entry`` with the plan, ``args(addresses of the inputs,
        then of the results)`` and the stream.  Returns the results."""
        self._need(entry, entry[len("cmpc_"):])
        inputs, results = spec
        if out is None:
            out = tuple(torch.empty(shape, dtype=dtype, device=self.device)
                        for dtype, shape in results.values())
        elif len(out) != len(results):
            raise ValueError(f"out must hold {tuple(results)}")
        ptrs = [self._address(t, name, *inputs[name]) for name, t in zip(inputs, tensors)]
        ptrs += [self._address(t, name, *results[name]) for name, t in zip(results, out)]
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, entry)(self._h, *args(*ptrs), _stream_ptr(stream, self.device))
        _check(self.lib, rc, entry)
        return tuple(out)

    def set_timing(self, enable: bool):
        _check(self.lib, self.lib.cmpc_plan_set_timing(self._h, int(bool(enable))),
               "cmpc_plan_set_timing")

    def set_team(self, max_batch: int):
        """Small-batch (team) mode for solves of B <= max_batch: four waves per QP.
        -1 = automatic (B <= 4 x CUs, the default), 0 = off (cmpc_plan_set_team)."""
        _check(self.lib, self.lib.cmpc_plan_set_team(self._h, int(max_batch)),
               "cmpc_plan_set_team")

    def team_batch(self) -> int:
        """The largest batch solved in team mode (cmpc_plan_team_batch)."""
        v = ctypes.c_int64()
        _check(self.lib, self.lib.cmpc_plan_team_batch(self._h, ctypes.byref(v)),
               "cmpc_plan_team_batch")
        return int(v.value)

    def set_heavy_first(self, min_batch: int):
        """Submit the NC 144 / 160 register class first for solves of B >= min_batch: -1 =
        automatic (B > 16 x CUs, the default), 0 = never (cmpc_plan_set_heavy_first)."""
        _check(self.lib, self.lib.cmpc_plan_set_heavy_first(self._h, int(min_batch)),
               "cmpc_plan_set_heavy_first")

    def heavy_first_batch(self) -> int:
        """The smallest batch that submits the NC 144 / 160 class first, 0 = never
        (cmpc_plan_heavy_first_batch)."""
        v = ctypes.c_int64()
        _check(self.lib, self.lib.cmpc_plan_heavy_first_batch(self._h, ctypes.byref(v)),
               "cmpc_plan_heavy_first_batch")
        return int(v.value)

    def solve_kernels(self, B: int) -> list:
        """Names of the solve kernels a batch of B launches, per timing slot (None: slot not
        launched), as cmpc_plan_solve_kernel reports them."""
        out = []
        for k in range(_lib.NUM_SOLVE_KERNELS):
            r = self.lib.cmpc_plan_solve_kernel(self._h, int(B), k)
            out.append(r.decode() if r else None)
        return out

    def stats(self, reset: bool = False) -> dict:
        """Acceptance statistics since plan creation or the last reset (cmpc_plan_stats):
        loose acceptances and the answers returned as status 2 by the certified bound or a
        stalled downdated refinement.  Synchronises the device."""
        keys = ("loose", "status2_cert", "guard_refactors")
        v = (ctypes.c_uint64 * _lib.NUM_STATS)()
        _check(self.lib, self.lib.cmpc_plan_stats(self._h, v, int(bool(reset))), "cmpc_plan_stats")
        return {k: int(x) for k, x in zip(keys, list(v))}

    def timing_read(self):
        """-> (ms_per_kernel, calls_per_kernel) of the solve kernels since the last read, one
        entry per timing slot (_lib.KERNEL_BINS: 0 = NC 128 + 96, 1 = NC 160 + 144, 2 = NC 192)."""
        ms = (ctypes.c_float * _lib.NUM_SOLVE_KERNELS)()
        calls = (ctypes.c_int32 * _lib.NUM_SOLVE_KERNELS)()
        _check(self.lib, self.lib.cmpc_plan_timing_read(self._h, ms, calls),
               "cmpc_plan_timing_read")
        return list(ms), list(calls)

    def solve(self, Ad, Bd, gd, x0, xref, contact, out=None, stream=None, w_init=None,
              y_init=None, y_out=None, lam_init=None, lam_out=None, mu=None, fz_min=None,
              Q=None, R=None):
        """Solve B instances; all inputs are device tensors (layouts: include/cmpc.h).

        Returns (w (B, 24N) fp32, status (B,) int32, iters (B,) int32).  Asynchronous on
        ``stream`` (default: torch's current stream).  Every option goes through one entry,
        cmpc_solve_io_run (include/cmpc.h).

        Warm start (the reference's x0 / lam_x0 warm start,
        centroidal_mpc.py:91-95): ``w_init`` (B, 24N) a previous w, ``y_init`` (B, 12N) a
        previous dual.  ``y_out`` (B, 12N) receives the dual at the returned forces; pass
        ``y_out=True`` to allocate it, in which case the return is (w, status, iters, y).

        Reference multipliers (centroidal_mpc.py:91-95, 108-110):
        ``lam_init`` (B, 52N) warm duals [lam_x | lam_a] in CasADi's layout and convention,
        ``lam_out`` (B, 52N) the multipliers of the returned point (``lam_out=True``
        allocates it; the return is then (w, status, iters, lam)).  Not combinable with
        y_init / y_out.

        Per-instance terrain: ``mu`` (B,) the friction coefficient and
        ``fz_min`` (B,) the stance normal-force floor of each instance, fp32 device tensors;
        None takes the plan's constant.  They combine with every option above.  The kernels
        read them when they run, so a captured graph sees values written in place since.  An
        instance whose entry is invalid (mu not finite or <= 0, fz_min not finite) returns
        status -10 with zero forces; the others are unaffected.

        Per-instance cost weights: ``Q`` (B, 12) the state-weight diagonal and
        ``R`` (B, 12) the input-weight diagonal of each instance, fp32 device tensors in the
        order of ``SolverParams.Q`` / ``R``; None takes the plan's constants.  Same rules: read
        when the kernels run, combinable with every option, and a row with a Q entry negative
        or not finite or an R entry <= 0 or not finite returns status -10 with zero forces."""
        self._need("cmpc_solve_io_run", "solve")
        B = Ad.shape[0]
        spec = _solve_spec(B, self.params.N)

        def empty(name):
            dtype, shape = spec[name]
            return torch.empty(shape, dtype=dtype, device=self.device)
        ret_y, ret_l = y_out is True, lam_out is True
        if ret_y:
            y_out = empty("y_out")
        if ret_l:
            lam_out = empty("lam_out")
        if (lam_init is not None or lam_out is not None) and (y_init is not None or y_out is not None):
            raise ValueError("lam_init/lam_out (reference layout) and y_init/y_out "
                             "(cmpc layout) are exclusive")
        w, status, iters = (empty("w"), empty("status"), empty("iters")) if out is None else out
        io = _lib.CSolveIO()
        io.size = ctypes.sizeof(_lib.CSolveIO)
        self._fill_io(io, spec,
                      _problem(Ad, Bd, gd, x0, xref, contact, w=w, status=status, iters=iters),
                      dict(w_init=w_init, y_init=y_init, lam_init=lam_init, y_out=y_out,
                           lam_out=lam_out, mu=mu, fz_min=fz_min, Q=Q, R=R), {"w": "w_out"})
        self._run_io("cmpc_solve_io_run", io, B, stream)
        return (w, status, iters) + ((y_out,) if ret_y else ()) + ((lam_out,) if ret_l else ())

    def kkt(self, Ad, Bd, gd, x0, xref, contact, w, lam=None, mu=None, fz_min=None, Q=None,
            R=None, face_tol=None, out=None, stream=None):
        """Cost and KKT residuals of B points on the device (cmpc_kkt_run, include/cmpc.h).

        ``Ad`` .. ``contact`` and ``mu`` / ``fz_min`` / ``Q`` / ``R`` as for :meth:`solve`; ``w``
        (B, 24N) fp32 the points (a solve's w); ``lam`` (B, 52N) fp32 their multipliers in the
        reference layout (a solve's ``lam_out``), or None to recover them from ``w`` on the
        device (the rule of :func:`cmpc.duals.recover` with ``tol = face_tol``, None = 1e-6):
        the mode for a plain or warm solve's output.  Returns a (B, 4) float64 device tensor
        with the columns :data:`KKT_COLUMNS`: the reference's cost 1/2 w'Hw + g'w and the
        stationarity, primal and complementarity residuals of ``oracle.mpc_qp.kkt_residuals``
        (``comp`` is +inf when a multiplier has the sign of an infinite bound).  An instance
        with an invalid mu / fz_min entry or Q / R row gets four NaNs.  Asynchronous on
        ``stream`` (default: torch's current stream), no allocation when ``out`` is given,
        graph-capturable; the inputs are not modified and B is not limited by max_batch."""
        self._need("cmpc_kkt_run", "kkt")
        N = self.params.N
        B = Ad.shape[0]
        if B < 1:
            raise ValueError("kkt needs at least one instance")
        io = _lib.CKktIO()
        io.size = ctypes.sizeof(_lib.CKktIO)
        self._fill_io(io, _eval_spec(B, N), _problem(Ad, Bd, gd, x0, xref, contact, w=w),
                      dict(lam=lam, mu=mu, fz_min=fz_min, Q=Q, R=R))
        if out is None:
            out = torch.empty((B, 4), dtype=torch.float64, device=self.device)
        io.res = self._address(out, "out", torch.float64, (B, 4))
        io.face_tol = 0.0 if face_tol is None else float(face_tol)
        self._run_io("cmpc_kkt_run", io, B, stream)
        return out

    def gain(self, Ad, Bd, gd, x0, xref, contact, w=None, faces=None, mu=None, fz_min=None,
             Q=None, R=None, face_tol=None, want=("K",), out=None, stream=None):
        """Feedback gain and value function of B solved instances on the device (cmpc_gain_run,
        include/cmpc.h): on the faces its forces hold the MPC law is affine, u0 = K x0 + kappa.

        ``Ad`` .. ``contact`` and ``mu`` / ``fz_min`` / ``Q`` / ``R`` as for :meth:`solve`.  The
        held faces are read off ``w`` (B, 24N) fp32, a solve's w, by the rule of
        :func:`cmpc.duals.recover` with ``tol = face_tol`` (None = 1e-6), or given as ``faces``
        (B, N, 4) uint8 masks (bits ``_lib.FACE_*``; ``w`` is then ignored).  ``want`` names the
        results, a subset of ``("K", "Vx", "Vxx", "u_star", "faces")``; ``K`` is always computed.
        Returns a dict of device tensors: ``K`` (B, 12, 12) float64 = d u0 / d x0, ``Vx`` (B, 12)
        and ``Vxx`` (B, 12, 12) the gradient and Hessian in x0 of the optimal cost, ``u_star``
        (B, 12N) float64 the optimum on the held faces, ``faces`` (B, N, 4) uint8 the masks used.
        An instance with an inconsistent mask or an invalid mu / fz_min entry or Q / R row gets
        NaN (0xFF in ``faces``).  ``out`` is a dict of preallocated tensors for some or all of
        the wanted names.  Asynchronous on ``stream`` (default: torch's current stream), no
        allocation when every wanted name is in ``out``, graph-capturable; the inputs are not
        modified and B is not limited by max_batch."""
        self._need("cmpc_gain_run", "gain")
        want = tuple(want)
        unknown = [n for n in want if n not in _lib.GAIN_OUTPUTS]
        if unknown:
            raise ValueError(f"gain: unknown result {unknown}; choose from {_lib.GAIN_OUTPUTS}")
        if w is None and faces is None:
            raise ValueError("gain needs w or faces: one must name the held faces")
        N = self.params.N
        B = Ad.shape[0]
        if B < 1:
            raise ValueError("gain needs at least one instance")
        f64, u8 = torch.float64, torch.uint8
        io = _lib.CGainIO()
        io.size = ctypes.sizeof(_lib.CGainIO)
        self._fill_io(io, _eval_spec(B, N), _problem(Ad, Bd, gd, x0, xref, contact),
                      dict(w=w, faces=faces, mu=mu, fz_min=fz_min, Q=Q, R=R))
        spec = dict(K=("K", f64, (B, 12, 12)), Vx=("Vx", f64, (B, 12)), Vxx=("Vxx", f64, (B, 12, 12)),
                    u_star=("u_star", f64, (B, 12 * N)), faces=("faces_out", u8, (B, N, 4)))
        res = self._results(io, spec, want, ("K",), out, self.device)
        io.face_tol = 0.0 if face_tol is None else float(face_tol)
        self._run_io("cmpc_gain_run", io, B, stream)
        return res

    def vjp(self, Ad, Bd, gd, x0, xref, contact, gw, w=None, faces=None, mu=None, fz_min=None,
            Q=None, R=None, face_tol=None, want=("x0",), out=None, stream=None):
        """Gradients of a loss through B solved instances on the device (cmpc_vjp_run,
        include/cmpc.h): the backward pass of the MPC as a differentiable layer.

        ``Ad`` .. ``contact``, ``mu`` / ``fz_min`` / ``Q`` / ``R``, ``w`` / ``faces`` and
        ``face_tol`` as for :meth:`gain`; ``gw`` (B, 24N) fp32 is dL/dw in w's layout, states
        then forces.  ``want`` names the inputs whose gradient is wanted, a non-empty subset of
        ``("x0", "xref", "gd", "Q", "R", "mu", "fz_min", "Ad", "Bd")``; work that only the others
        need is skipped, and a result does not depend on what else is asked for.  Returns a dict
        of float64 device tensors of the inputs' shapes (``Q`` / ``R`` (B, 12) and ``mu`` /
        ``fz_min`` (B,) whether the values came from the plan or from a row).  The gradient is
        that of the fp64 optimum on the held faces, the face set fixed (:meth:`gain`'s
        ``u_star`` and its rollout).  An instance with an inconsistent mask or an invalid mu /
        fz_min entry or Q / R row gets NaN.  ``out`` is a dict of preallocated tensors for some
        or all of the wanted names.  Asynchronous on ``stream`` (default: torch's current
        stream), no allocation when every wanted name is in ``out``, graph-capturable; the
        inputs are not modified and B is not limited by max_batch."""
        self._need("cmpc_vjp_run", "vjp")
        want = tuple(want)
        unknown = [n for n in want if n not in _lib.VJP_OUTPUTS]
        if unknown or not want:
            raise ValueError(f"vjp: want {want} must be a non-empty subset of {_lib.VJP_OUTPUTS}")
        if w is None and faces is None:
            raise ValueError("vjp needs w or faces: one must name the held faces")
        N = self.params.N
        B = Ad.shape[0]
        if B < 1:
            raise ValueError("vjp needs at least one instance")
        f64 = torch.float64
        io = _lib.CVjpIO()
        io.size = ctypes.sizeof(_lib.CVjpIO)
        self._fill_io(io, _eval_spec(B, N), _problem(Ad, Bd, gd, x0, xref, contact, gw=gw),
                      dict(w=w, faces=faces, mu=mu, fz_min=fz_min, Q=Q, R=R))
        shapes = dict(x0=(B, 12), xref=(B, N, 12), gd=(B, 12), Q=(B, 12), R=(B, 12), mu=(B,),
                      fz_min=(B,), Ad=(B, 12, 12), Bd=(B, N, 12, 12))
        spec = {name: ("g_" + name, f64, shape) for name, shape in shapes.items()}
        res = self._results(io, spec, want, (), out, self.device)
        io.face_tol = 0.0 if face_tol is None else float(face_tol)
        self._run_io("cmpc_vjp_run", io, B, stream)
        return res

    def jvp(self, Ad, Bd, gd, x0, xref, contact, tangents, w=None, faces=None, mu=None,
            fz_min=None, Q=None, R=None, face_tol=None, out=None, stream=None):
        """Forward-mode derivative of B solved instances on the device (cmpc_jvp_run,
        include/cmpc.h): how the whole answer moves with the inputs.

        ``Ad`` .. ``contact``, ``mu`` / ``fz_min`` / ``Q`` / ``R``, ``w`` / ``faces`` and
        ``face_tol`` as for :meth:`gain`.  ``tangents`` is a non-empty dict from input name, one of
        ``("x0", "xref", "gd", "Q", "R", "mu", "fz_min", "Ad", "Bd")``, to an fp32 device tensor
        of that input's shape (``Q`` / ``R`` (B, 12) and ``mu`` / ``fz_min`` (B,) whether the
        values come from the plan or from a row); an input that is not named does not move, and
        work that only absent tangents need is skipped.  Returns ``dw`` (B, 24N) float64 in w's
        layout, states then forces: the directional derivative of the fp64 optimum on the held
        faces, the face set fixed (:meth:`gain`'s ``u_star`` and its rollout) -- :meth:`vjp`'s
        Jacobian applied from the other side.  An instance with an inconsistent mask or an
        invalid mu / fz_min entry or Q / R row gets a row of NaN.  ``out`` is a preallocated
        ``dw``.  Asynchronous on ``stream`` (default: torch's current stream), no allocation
        when ``out`` is given, graph-capturable; the inputs are not modified and B is not
        limited by max_batch."""
        self._need("cmpc_jvp_run", "jvp")
        tangents = dict(tangents)
        unknown = [n for n in tangents if n not in _lib.JVP_TANGENTS]
        if unknown or not tangents:
            raise ValueError(f"jvp: tangents {tuple(tangents)} must name a non-empty subset of "
                             f"{_lib.JVP_TANGENTS}")
        if w is None and faces is None:
            raise ValueError("jvp needs w or faces: one must name the held faces")
        N = self.params.N
        B = Ad.shape[0]
        if B < 1:
            raise ValueError("jvp needs at least one instance")
        io = _lib.CJvpIO()
        io.size = ctypes.sizeof(_lib.CJvpIO)
        self._fill_io(io, _eval_spec(B, N), _problem(Ad, Bd, gd, x0, xref, contact),
                      dict(w=w, faces=faces, mu=mu, fz_min=fz_min, Q=Q, R=R))
        shapes = dict(x0=(B, 12), xref=(B, N, 12), gd=(B, 12), Q=(B, 12), R=(B, 12), mu=(B,),
                      fz_min=(B,), Ad=(B, 12, 12), Bd=(B, N, 12, 12))
        self._fill_io(io, {"d_" + n: (torch.float32, s) for n, s in shapes.items()},
                      {"d_" + n: t for n, t in tangents.items()}, {})
        if out is None:
            out = torch.empty((B, 24 * N), dtype=torch.float64, device=self.device)
        io.dw = self._address(out, "out", torch.float64, (B, 24 * N))
        io.face_tol = 0.0 if face_tol is None else float(face_tol)
        self._run_io("cmpc_jvp_run", io, B, stream)
        return out

    def refine(self, Ad, Bd, gd, x0, xref, contact, w=None, faces=None, mu=None, fz_min=None,
               Q=None, R=None, face_tol=0.0, max_rounds=8, prim_tol=0.0, dual_tol=0.0, w_out=None,
               status=None, want=("info", "res"), out=None, stream=None):
        """Certified float64 refinement of B solved instances on the device (cmpc_refine_run,
        include/cmpc.h): a primal-dual active-set loop around :meth:`gain`'s ``u_star`` that
        replaces an answer only when the float64 KKT conditions hold on the whole QP.

        ``Ad`` .. ``contact``, ``mu`` / ``fz_min`` / ``Q`` / ``R``, ``w`` / ``faces`` and
        ``face_tol`` (0 = 1e-6) as for :meth:`gain`; with ``faces`` given, ``w`` is still the
        answer the error is measured from.  ``max_rounds`` (0..16) limits the repairs, 0 checks
        only; ``prim_tol`` / ``dual_tol`` (0 = 1e-9) are the relative thresholds of a violated
        face and of a negative multiplier.  ``w_out`` (B, 24N) fp32, which may be ``w`` itself,
        receives the fp32 rounding of the certified point in the rows that were certified and
        is left untouched, bit for bit, in every other row; ``status`` (B,) int32 is set to 1 in
        the certified rows and left untouched otherwise.  ``want`` names the results, a subset
        of ``("info", "res", "w64", "lam", "faces")``; ``info`` is always computed.  Returns a
        dict of device tensors: ``info`` (B,) int32, r >= 0 = certified after r repairs,
        ``_lib.REFINE_INVALID`` / ``REFINE_ROUNDS`` / ``REFINE_CYCLE`` otherwise; ``res`` (B, 3)
        float64, the largest violation / us, the most negative held multiplier / gs and
        max|u - u_in| / max(1, max|u_in|) (NaN without ``w``), on a certified row the measured
        error of the answer given; ``w64`` (B, 24N) float64 the last round's point; ``lam``
        (B, 52N) float64 its multipliers ``[lam_x | lam_a]`` in the layout of a solve's
        ``lam_out``; ``faces`` (B, N, 4) uint8 its masks.  An invalid instance (an invalid mu /
        fz_min entry or Q / R row, a given mask with both signs of an axis) gets NaN (0xFF in
        ``faces``).  ``out`` is a dict of preallocated tensors for some or all of the wanted
        names.  Asynchronous on ``stream`` (default: torch's current stream), no allocation when
        every wanted name is in ``out``, graph-capturable; B is not limited by max_batch."""
        self._need("cmpc_refine_run", "refine")
        want = tuple(want)
        unknown = [n for n in want if n not in _lib.REFINE_OUTPUTS]
        if unknown:
            raise ValueError(f"refine: unknown result {unknown}; choose from {_lib.REFINE_OUTPUTS}")
        if w is None and faces is None:
            raise ValueError("refine needs w or faces: one must name the held faces")
        N = self.params.N
        B = Ad.shape[0]
        if B < 1:
            raise ValueError("refine needs at least one instance")
        f64, u8, i32 = torch.float64, torch.uint8, torch.int32
        io = _lib.CRefineIO()
        io.size = ctypes.sizeof(_lib.CRefineIO)
        self._fill_io(io, _eval_spec(B, N), _problem(Ad, Bd, gd, x0, xref, contact),
                      dict(w=w, faces=faces, w_out=w_out, status=status, mu=mu, fz_min=fz_min,
                           Q=Q, R=R))
        spec = dict(info=("info", i32, (B,)), res=("res", f64, (B, 3)),
                    w64=("w64", f64, (B, 24 * N)), lam=("lam_out", f64, (B, 52 * N)),
                    faces=("faces_out", u8, (B, N, 4)))
        res = self._results(io, spec, want, ("info",), out, self.device)
        io.face_tol = float(face_tol)
        io.max_rounds = int(max_rounds)
        io.prim_tol, io.dual_tol = float(prim_tol), float(dual_tol)
        self._run_io("cmpc_refine_run", io, B, stream)
        return res

    def build_dynamics(self, mass, inertia, r_feet, xref, dt, out=None, stream=None):
        """Discrete dynamics (Ad, Bd, gd) of B robots on the device -- the reference's
        ComTraj._continuousDynamics + _discreteDynamics (com_trajectory.py:221-286) in closed
        form.  mass (B,), inertia (B,3,3) I_com_world, r_feet (B,N,4,3) COM->foot lever arms
        (legs FL FR RL RR), xref (B,N,12) as for solve(); all fp32 device tensors."""
        B = mass.shape[0]
        return self._pipeline("cmpc_build_dynamics", _dynamics_spec(B, self.params.N),
                              (mass, inertia, r_feet, xref), out, stream, lambda *p: (B, dt, *p))

    def dynamics_vjp(self, mass, inertia, r_feet, xref, dt, g_Ad=None, g_Bd=None, want=None,
                     out=None, stream=None):
        """Gradients of a loss through :meth:`build_dynamics` on the device
        (cmpc_dynamics_vjp_run, include/cmpc.h): from dL/dAd and dL/dBd to the gradients in the
        mass, the world-frame inertia, the foot levers and the mean reference yaw.

        ``mass`` .. ``xref`` and ``dt`` as for :meth:`build_dynamics`; ``g_Ad`` (B, 12, 12) and
        ``g_Bd`` (B, N, 12, 12) are float64 device tensors -- what :meth:`vjp` returns for
        ``want=("Ad", "Bd")`` -- of which one may be None (zeros).  ``want`` names the results, a
        non-empty subset of ``("mass", "inertia", "r_feet", "yaw")`` (None: all four); a result
        does not depend on what else is asked for, and the parts of ``g_Bd`` that only the
        others need are not read.  Returns a dict of float64 device tensors: ``mass`` (B,),
        ``inertia`` (B, 3, 3) with its nine entries independent, ``r_feet`` (B, N, 4, 3) and
        ``yaw`` (B,), the gradient in the mean of ``xref[:, :, 5]`` -- every ``xref[b, k, 5]``
        gets ``yaw[b] / N``, every other entry of ``xref`` zero.  The gradient is that of the
        closed form in fp64 on the fp32 inputs, not of its fp32-rounded outputs.  ``out`` is a
        dict of preallocated tensors for some or all of the wanted names.  Asynchronous on
        ``stream`` (default: torch's current stream), no allocation when every wanted name is in
        ``out``, graph-capturable; B is not limited by max_batch."""
        self._need("cmpc_dynamics_vjp_run", "dynamics_vjp")
        want = _lib.DYNAMICS_VJP_OUTPUTS if want is None else tuple(want)
        unknown = [n for n in want if n not in _lib.DYNAMICS_VJP_OUTPUTS]
        if unknown or not want:
            raise ValueError(f"dynamics_vjp: want {want} must be a non-empty subset of "
                             f"{_lib.DYNAMICS_VJP_OUTPUTS}")
        if g_Ad is None and g_Bd is None:
            raise ValueError("dynamics_vjp needs g_Ad or g_Bd: one must be given")
        B = mass.shape[0]
        N = self.params.N
        grads, results, _, _ = _dynamics_grad_spec(B, N)
        io = _lib.CDynamicsVjpIO()
        io.size = ctypes.sizeof(_lib.CDynamicsVjpIO)
        self._fill_io(io, _dynamics_spec(B, N)[0],
                      dict(mass=mass, inertia=inertia, r_feet=r_feet, xref=xref), {})
        self._fill_io(io, grads, {}, dict(g_Ad=g_Ad, g_Bd=g_Bd))
        res = self._results(io, results, want, (), out, self.device)
        io.dt = float(dt)
        self._run_io("cmpc_dynamics_vjp_run", io, B, stream)
        return res

    def dynamics_jvp(self, mass, inertia, r_feet, xref, dt, tangents, want=("Ad", "Bd"), out=None,
                     stream=None):
        """Forward-mode derivative of :meth:`build_dynamics` on the device
        (cmpc_dynamics_jvp_run, include/cmpc.h): how ``Ad`` and ``Bd`` move with the mass, the
        inertia, the foot levers and the reference yaw.

        ``mass`` .. ``xref`` and ``dt`` as for :meth:`build_dynamics`.  ``tangents`` is a
        non-empty dict from input name, one of ``("mass", "inertia", "r_feet", "xref")``, to an
        fp32 device tensor of that input's shape; an input that is not named does not move, and
        of ``xref``'s tangent only column 5 (the yaw) is read.  ``want`` is a non-empty subset of
        ``("Ad", "Bd")``.  Returns a dict of fp32 device tensors of those shapes, the fp64
        derivative rounded once -- what :meth:`jvp` takes as its ``Ad`` and ``Bd`` tangents;
        ``Ad`` is exactly zero outside its rows 3-4, columns 9-10, and ``gd`` does not move.  A
        result does not depend on whether the other is asked for.  ``out`` is a dict of
        preallocated tensors for some or all of the wanted names.  Asynchronous on ``stream``
        (default: torch's current stream), no allocation when every wanted name is in ``out``,
        graph-capturable; B is not limited by max_batch."""
        self._need("cmpc_dynamics_jvp_run", "dynamics_jvp")
        tangents, want = dict(tangents), tuple(want)
        unknown = [n for n in tangents if n not in _lib.DYNAMICS_JVP_TANGENTS]
        if unknown or not tangents:
            raise ValueError(f"dynamics_jvp: tangents {tuple(tangents)} must name a non-empty "
                             f"subset of {_lib.DYNAMICS_JVP_TANGENTS}")
        if not want or [n for n in want if n not in _lib.DYNAMICS_JVP_OUTPUTS]:
            raise ValueError(f"dynamics_jvp: want {want} must be a non-empty subset of "
                             f"{_lib.DYNAMICS_JVP_OUTPUTS}")
        B = mass.shape[0]
        N = self.params.N
        _, _, moves, results = _dynamics_grad_spec(B, N)
        io = _lib.CDynamicsJvpIO()
        io.size = ctypes.sizeof(_lib.CDynamicsJvpIO)
        self._fill_io(io, _dynamics_spec(B, N)[0],
                      dict(mass=mass, inertia=inertia, r_feet=r_feet, xref=xref), {})
        self._fill_io(io, moves, {"d_" + n: t for n, t in tangents.items()}, {})
        res = self._results(io, results, want, (), out, self.device)
        io.dt = float(dt)
        self._run_io("cmpc_dynamics_jvp_run", io, B, stream)
        return res

    def generate_traj(self, x0, pos_des, cmd, t_now, gait, foot_lever, hip, dt, out=None,
                      stream=None):
        """Reference trajectory, contact table and foot levers of B robots on the device -- the
        reference's ComTraj.generate_traj (com_trajectory.py:27-207) up to the dynamics
        (cmpc_generate_traj, include/cmpc.h).  x0 (B,12) fp32; pos_des (B,3) fp64, updated in
        place (ComTraj.pos_des_world); cmd (B,4) fp32 [vx_body, vy_body, z_des, yaw_rate];
        t_now (B,) fp64; gait (B,6) fp64 [period, duty, 4 phase offsets]; foot_lever (B,4,3)
        fp32; hip (4,3) fp32.  Returns (xref (B,N,12), contact (B,4,N) uint8,
        r_feet (B,N,4,3))."""
        B = x0.shape[0]
        return self._pipeline("cmpc_generate_traj", _traj_spec(B, self.params.N),
                              (x0, pos_des, cmd, t_now, gait, foot_lever, hip), out, stream,
                              lambda *p: (B, dt, *p))

    def traj_vjp(self, x0, pos_des, cmd, t_now, gait, hip, dt, g_xref=None, g_r_feet=None,
                 g_yaw=None, g_pos_des=None, want=None, out=None, stream=None):
        """Gradients of a loss through :meth:`generate_traj` on the device (cmpc_traj_vjp_run,
        include/cmpc.h): from dL/dxref, dL/dr_feet, dL/d(mean reference yaw) and the gradient in
        the desired position it leaves to the gradients in the state, the desired position, the
        command and the current foot levers.

        ``x0`` .. ``hip`` and ``dt`` as for :meth:`generate_traj`, without ``foot_lever`` (its
        values are not needed); ``pos_des`` is the value BEFORE :meth:`generate_traj` overwrote it
        (with the clamped value a clamped robot reads as unclamped) and is not modified.
        ``g_xref`` (B, N, 12) -- what :meth:`vjp` returns for ``want=("xref",)`` -- ``g_r_feet``
        (B, N, 4, 3) and ``g_yaw`` (B,) -- what :meth:`dynamics_vjp` returns, ``g_yaw / N`` being
        added to every step's yaw gradient -- and ``g_pos_des`` (B, 3), the gradient in the
        desired position after the clamp, are float64 device tensors; each may be None (zeros),
        one must be given.  ``want`` names the results, a non-empty subset of ``("x0", "pos_des",
        "cmd", "foot_lever")`` (None: all four); a result does not depend on what else is asked
        for.  Returns a dict of float64 device tensors of the inputs' shapes; ``x0`` is written
        whole, zero outside its entries 0, 1, 3, 4, 5.  The contact pattern and the branch of the
        clamp are held fixed, and the gradient is that of the fp64 function on the fp32 inputs,
        not of its fp32-rounded outputs.  ``out`` is a dict of preallocated tensors for some or
        all of the wanted names.  Asynchronous on ``stream`` (default: torch's current stream),
        no allocation when every wanted name is in ``out``, graph-capturable; B is not limited by
        max_batch."""
        self._need("cmpc_traj_vjp_run", "traj_vjp")
        want = _lib.TRAJ_VJP_OUTPUTS if want is None else tuple(want)
        if not want or [n for n in want if n not in _lib.TRAJ_VJP_OUTPUTS]:
            raise ValueError(f"traj_vjp: want {want} must be a non-empty subset of "
                             f"{_lib.TRAJ_VJP_OUTPUTS}")
        given = dict(g_xref=g_xref, g_r_feet=g_r_feet, g_yaw=g_yaw, g_pos_des_out=g_pos_des)
        if all(t is None for t in given.values()):
            raise ValueError("traj_vjp needs g_xref, g_r_feet, g_yaw or g_pos_des: one must be given")
        B = x0.shape[0]
        inputs, grads, results, _, _ = _traj_grad_spec(B, self.params.N)
        io = _lib.CTrajVjpIO()
        io.size = ctypes.sizeof(_lib.CTrajVjpIO)
        self._fill_io(io, inputs, dict(x0=x0, pos_des=pos_des, cmd=cmd, t_now=t_now, gait=gait,
                                       hip=hip), {})
        self._fill_io(io, grads, {}, given)
        res = self._results(io, results, want, (), out, self.device)
        io.dt = float(dt)
        self._run_io("cmpc_traj_vjp_run", io, B, stream)
        return res

    def traj_jvp(self, x0, pos_des, cmd, t_now, gait, hip, dt, tangents,
                 want=("xref", "r_feet", "pos_des"), out=None, stream=None):
        """Forward-mode derivative of :meth:`generate_traj` on the device (cmpc_traj_jvp_run,
        include/cmpc.h): how ``xref``, ``r_feet`` and the desired position it leaves move with
        the state, the desired position, the command and the current foot levers.

        ``x0`` .. ``hip`` and ``dt`` as for :meth:`traj_vjp` (``pos_des`` before the clamp, not
        modified).  ``tangents`` is a non-empty dict from input name, one of ``("x0", "pos_des",
        "cmd", "foot_lever")``, to a device tensor of that input's shape and dtype (fp32,
        ``pos_des`` float64); an input that is not named does not move.  ``want`` is a non-empty
        subset of ``("xref", "r_feet", "pos_des")``.  Returns a dict: ``xref`` (B, N, 12) and
        ``r_feet`` (B, N, 4, 3) fp32, the fp64 derivative rounded once -- what :meth:`jvp` and
        :meth:`dynamics_jvp` take as those tangents -- and ``pos_des`` (B, 3) float64.  A swing
        lever's tangent and columns 3, 4, 8, 9, 10 of ``xref``'s are exactly zero.  A result does
        not depend on what else is asked for.  ``out`` is a dict of preallocated tensors for some
        or all of the wanted names.  Asynchronous on ``stream`` (default: torch's current
        stream), no allocation when every wanted name is in ``out``, graph-capturable; B is not
        limited by max_batch."""
        self._need("cmpc_traj_jvp_run", "traj_jvp")
        tangents, want = dict(tangents), tuple(want)
        if not tangents or [n for n in tangents if n not in _lib.TRAJ_JVP_TANGENTS]:
            raise ValueError(f"traj_jvp: tangents {tuple(tangents)} must name a non-empty subset "
                             f"of {_lib.TRAJ_JVP_TANGENTS}")
        if not want or [n for n in want if n not in _lib.TRAJ_JVP_OUTPUTS]:
            raise ValueError(f"traj_jvp: want {want} must be a non-empty subset of "
                             f"{_lib.TRAJ_JVP_OUTPUTS}")
        B = x0.shape[0]
        inputs, _, _, moves, results = _traj_grad_spec(B, self.params.N)
        io = _lib.CTrajJvpIO()
        io.size = ctypes.sizeof(_lib.CTrajJvpIO)
        self._fill_io(io, inputs, dict(x0=x0, pos_des=pos_des, cmd=cmd, t_now=t_now, gait=gait,
                                       hip=hip), {})
        self._fill_io(io, moves, {"d_" + n: t for n, t in tangents.items()}, {})
        res = self._results(io, results, want, (), out, self.device)
        io.dt = float(dt)
        self._run_io("cmpc_traj_jvp_run", io, B, stream)
        return res

    def leg_torque(self, t, gait, force, J_foot, J_full, M, C, g, dq, Jdot_dq, foot_pos, foot_vel,
                   body, hip, state, tau_max=45.0, out=None, stream=None):
        """The reference's leg controller tick for B robots (cmpc_leg_torque, include/cmpc.h;
        leg_controller.py:43-112 + the clip of test_MPC.py:227-228).  ``force`` is (B, 12) fp32
        or a (B, >=12) fp32 view whose rows start at U[:, 0] (e.g. w[:, 12N:]); everything else
        fp64 device tensors; ``state`` (B, 4, 8) is updated in place (initialise with
        :func:`leg_state`).  Returns tau (B, 12) fp64."""
        B = t.shape[0]
        _force_rows(force, B, self.device)
        return self._pipeline(
            "cmpc_leg_torque", _leg_spec(B),
            (t, gait, J_foot, J_full, M, C, g, dq, Jdot_dq, foot_pos, foot_vel, body, hip, state),
            None if out is None else (out,), stream,
            lambda t_, gait_, *p: (B, t_, gait_, force.data_ptr(), force.stride(0), *p[:12],
                                   tau_max, p[12]))[0]

    def srb_step(self, t_now, gait, mass, inertia_body, force, hip, x, feet, contact_state, nsub,
                 dt, stream=None, K=None, x_solve=None, contact=None, mu=None, fz_min=None,
                 wrench=None, force_out=None, fb_status=None):
        """``nsub`` substeps of ``dt`` of the single-rigid-body plant for B robots
        (cmpc_srb_step, include/cmpc.h).  t_now (B,) and gait (B, 6) fp64; mass (B,),
        inertia_body (B, 3, 3) and hip (4, 3) fp32; ``force`` as for :meth:`leg_torque`; x
        (B, 12) fp32, feet (B, 4, 3) fp32 and contact_state (B,) uint8 are updated in place.

        With any of the options the step is cmpc_srb_step_io_run's (include/cmpc.h).  ``K``
        (B, 12, 12) float64, :meth:`gain`'s ``K``, with ``x_solve`` (B, 12) fp32, the state the
        forces were solved from, and ``contact`` (B, 4, N) uint8, the solve's contact table: every
        substep applies ``force + K (x - x_solve)``, the legs the MPC planned in stance clamped to
        ``fz >= fz_min`` and ``|fx|, |fy| <= mu fz`` (``mu`` / ``fz_min``: (B,) fp32, None: the
        plan's constants).  A robot whose ``K`` is not finite or whose ``mu`` / ``fz_min`` is
        invalid holds ``force``.  ``wrench`` (B, 6) fp32: a world force at the COM and a world
        torque about it, held over the substeps.  ``force_out`` (B, 12) fp32 receives the forces
        of the last substep and ``fb_status`` (B,) uint8 0 (held), 1 (law applied) or 2 (applied
        and clamped)."""
        B = x.shape[0]
        _force_rows(force, B, self.device)
        options = dict(K=K, x_solve=x_solve, contact=contact, mu=mu, fz_min=fz_min, wrench=wrench,
                       force_out=force_out, fb_status=fb_status)
        if any(t is not None for t in options.values()):
            self._need("cmpc_srb_step_io_run", "srb_step")
            if K is not None and (x_solve is None or contact is None):
                raise ValueError("srb_step: K needs x_solve and contact")
            io = _lib.CSrbIO()
            self._srb_grad_io(io, _srb_spec(B)[0], t_now, gait, mass, inertia_body, force, hip, x,
                              feet, contact_state, nsub, dt)
            self._fill_io(io, _srb_io_spec(B, self.params.N), {}, options)
            self._run_io("cmpc_srb_step_io_run", io, B, stream)
            return
        self._pipeline(
            "cmpc_srb_step", _srb_spec(B),
            (t_now, gait, mass, inertia_body, hip, x, feet, contact_state), None, stream,
            lambda t_, gait_, mass_, inertia_, *p: (B, int(nsub), dt, t_, gait_, mass_, inertia_,
                                                    force.data_ptr(), force.stride(0), *p))

    def _srb_grad_io(self, io, inputs, t_now, gait, mass, inertia_body, force, hip, x, feet,
                     contact_state, nsub, dt):
        """The part of cmpc_srb_vjp_io and cmpc_srb_jvp_io that is cmpc_srb_step's arguments."""
        B = x.shape[0]
        _force_rows(force, B, self.device)
        io.size = ctypes.sizeof(type(io))
        self._fill_io(io, inputs, dict(t_now=t_now, gait=gait, mass=mass, inertia_body=inertia_body,
                                       hip=hip, x=x, feet=feet, contact_state=contact_state), {})
        io.force, io.force_stride = force.data_ptr(), force.stride(0)
        io.nsub, io.dt = int(nsub), float(dt)

    def srb_vjp(self, t_now, gait, mass, inertia_body, force, hip, x, feet, contact_state, nsub, dt,
                g_x=None, g_feet=None, want=None, out=None, stream=None):
        """Gradients of a loss through :meth:`srb_step` on the device (cmpc_srb_vjp_run,
        include/cmpc.h): from dL/dx' and dL/dfeet' to the gradients in the state, the feet, the
        held forces, the mass and the body inertia.

        ``t_now`` .. ``dt`` as for :meth:`srb_step`, but ``x``, ``feet`` and ``contact_state`` are
        the values BEFORE :meth:`srb_step` advanced them (keep a copy) and are not modified;
        ``nsub`` is in 1 .. 64.  ``g_x`` (B, 12) and ``g_feet`` (B, 4, 3) are float64 device
        tensors, the gradients in the advanced state and feet; each may be None (zeros), one must
        be given.  ``want`` names the results, a non-empty subset of ``("x", "feet", "force",
        "mass", "inertia_body")`` (None: all five); a result does not depend on what else is asked
        for.  Returns a dict of float64 device tensors of the inputs' shapes (``force``: packed
        (B, 12)).  The contact schedule depends on ``t_now``, ``gait`` and ``contact_state``
        alone, so the gradient is exact, that of the fp64 model on the fp32 inputs; there is none
        in ``t_now``, ``gait``, ``hip`` or ``dt``.  ``out`` is a dict of preallocated tensors for
        some or all of the wanted names.  Asynchronous on ``stream`` (default: torch's current
        stream), no allocation when every wanted name is in ``out``, graph-capturable; B is not
        limited by max_batch."""
        self._need("cmpc_srb_vjp_run", "srb_vjp")
        want = _lib.SRB_VJP_OUTPUTS if want is None else tuple(want)
        if not want or [n for n in want if n not in _lib.SRB_VJP_OUTPUTS]:
            raise ValueError(f"srb_vjp: want {want} must be a non-empty subset of "
                             f"{_lib.SRB_VJP_OUTPUTS}")
        given = dict(g_x_out=g_x, g_feet_out=g_feet)
        if all(t is None for t in given.values()):
            raise ValueError("srb_vjp needs g_x or g_feet: one must be given")
        B = x.shape[0]
        inputs, grads, results, _, _ = _srb_grad_spec(B)
        io = _lib.CSrbVjpIO()
        self._srb_grad_io(io, inputs, t_now, gait, mass, inertia_body, force, hip, x, feet,
                          contact_state, nsub, dt)
        self._fill_io(io, grads, {}, given)
        res = self._results(io, results, want, (), out, self.device)
        self._run_io("cmpc_srb_vjp_run", io, B, stream)
        return res

    def srb_jvp(self, t_now, gait, mass, inertia_body, force, hip, x, feet, contact_state, nsub, dt,
                tangents, want=("x", "feet"), out=None, stream=None):
        """Forward-mode derivative of :meth:`srb_step` on the device (cmpc_srb_jvp_run,
        include/cmpc.h): how the advanced state and feet move with the state, the feet, the held
        forces, the mass and the body inertia.

        ``t_now`` .. ``dt`` as for :meth:`srb_vjp` (``x``, ``feet`` and ``contact_state`` before
        the step, not modified).  ``tangents`` is a non-empty dict from input name, one of ``("x",
        "feet", "force", "mass", "inertia_body")``, to an fp32 device tensor of that input's shape
        (``force``: packed (B, 12)); an input that is not named does not move.  ``want`` is a
        non-empty subset of ``("x", "feet")``.  Returns a dict of fp32 tensors, the fp64
        derivative rounded once -- what :meth:`jvp` and :meth:`traj_jvp` take as the tangent of
        ``x0``.  A result does not depend on what else is asked for.  ``out`` is a dict of
        preallocated tensors for some or all of the wanted names.  Asynchronous on ``stream``
        (default: torch's current stream), no allocation when every wanted name is in ``out``,
        graph-capturable; B is not limited by max_batch."""
        self._need("cmpc_srb_jvp_run", "srb_jvp")
        tangents, want = dict(tangents), tuple(want)
        if not tangents or [n for n in tangents if n not in _lib.SRB_JVP_TANGENTS]:
            raise ValueError(f"srb_jvp: tangents {tuple(tangents)} must name a non-empty subset "
                             f"of {_lib.SRB_JVP_TANGENTS}")
        if not want or [n for n in want if n not in _lib.SRB_JVP_OUTPUTS]:
            raise ValueError(f"srb_jvp: want {want} must be a non-empty subset of "
                             f"{_lib.SRB_JVP_OUTPUTS}")
        B = x.shape[0]
        inputs, _, _, moves, results = _srb_grad_spec(B)
        io = _lib.CSrbJvpIO()
        self._srb_grad_io(io, inputs, t_now, gait, mass, inertia_body, force, hip, x, feet,
                          contact_state, nsub, dt)
        self._fill_io(io, moves, {"d_" + n: t for n, t in tangents.items()}, {})
        res = self._results(io, results, want, (), out, self.device)
        self._run_io("cmpc_srb_jvp_run", io, B, stream)
        return res


def leg_state(B: int, device="cuda") -> torch.Tensor:
    """Fresh leg-controller memory for cmpc_leg_torque: last mask 2 (LegController.__init__,
    leg_controller.py:40-41), everything else 0."""
    s = torch.zeros((B, 4, 8), dtype=torch.float64, device=device)
    s[:, :, 0] = 2.0
    return s


def to_device_batch(batch: dict, device="cuda") -> dict:
    """float64/uint8 numpy batch (cmpc.synth layout) -> contiguous device tensors."""
    out = {}
    for k in ("Ad", "Bd", "gd", "x0", "xref"):
        out[k] = torch.as_tensor(batch[k], dtype=torch.float32).contiguous().to(device)
    out["contact"] = torch.as_tensor(batch["contact"], dtype=torch.uint8).contiguous().to(device)
    # per-instance terrain (synth.make_terrain) and weights (synth.make_weights), when present
    for k in ("mu", "fz_min", "Q", "R"):
        if batch.get(k) is not None:
            out[k] = torch.as_tensor(batch[k], dtype=torch.float32).contiguous().to(device)
    return out


def solve_batch(batch: dict, params: Optional[SolverParams] = None, plan: Optional[Plan] = None):
    """Convenience: numpy batch in, (w, status, iters) numpy out (synchronises)."""
    plan = plan or Plan(params)
    d = to_device_batch(batch, plan.device)
    w, st, it = plan.solve(d["Ad"], d["Bd"], d["gd"], d["x0"], d["xref"], d["contact"],
                           mu=d.get("mu"), fz_min=d.get("fz_min"), Q=d.get("Q"), R=d.get("R"))
    torch.cuda.synchronize(plan.device)
    return w.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()
