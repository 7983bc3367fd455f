// cmpc_host.hip -- C-ABI (include/cmpc.h): plan management and kernel launches.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdlib.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "cmpc.h"
#include "cmpc_device.h"

#include "cmpc_wave.hip"      // solve kernels: same translation unit
#include "cmpc_dynamics.hip"  // QP-data (discrete dynamics) kernel
#include "cmpc_traj.hip"      // reference trajectory / contact table / foot levers kernel
#include "cmpc_leg.hip"       // leg controller (stance torque mapping, swing) kernel
#include "cmpc_sim.hip"       // single-rigid-body plant (closed-loop stand-in for MuJoCo)
#include "cmpc_kkt.hip"       // cost and KKT residuals of a batch of points
#include "cmpc_gain.hip"      // feedback gain and value function on the held faces
#include "cmpc_vjp.hip"       // gradients of a loss through the optimum on the held faces
#include "cmpc_refine.hip"    // certified float64 refinement around the optimum on the held faces
#include "cmpc_jvp.hip"       // forward-mode derivatives of the optimum on the held faces
#include "cmpc_dynamics_grad.hip"  // reverse- and forward-mode derivatives of the dynamics builder
#include "cmpc_traj_grad.hip"      // reverse- and forward-mode derivatives of the trajectory generator
#include "cmpc_sim_grad.hip"       // reverse- and forward-mode derivatives of the rigid-body plant
#include "cmpc_sim_fb.hip"         // the plant with the first-order force law and an external wrench

constexpr int kNumGroups = 3;  // solve kernels (register classes), see solve_group_kernel
static_assert(kNumGroups == CMPC_NUM_SOLVE_KERNELS, "one timing slot per solve kernel");

struct cmpc_plan {
  cmpc_params p;
  cmpc::KParams kp;
  int device;
  int cus = 0;      // compute units of the device
  int* d_counters = nullptr;  // counts[kNumBins], heads[kNumBins]
  unsigned long long* d_stats = nullptr;  // CMPC_NUM_STATS cumulative counters (cmpc_plan_stats)
  int* d_lists = nullptr;     // kNumBins * max_batch
  // per-wave park slabs; group k's region starts at work_off[k] (groups overlap)
  float* d_work = nullptr;
  size_t work_off[kNumGroups];
  int grid[kNumGroups];      // persistent grid of each group's one-wave kernel
  size_t slab[kNumGroups];   // park slab per wave (floats)
  // small batches (B <= team_max_batch): one kernel for all bins, kTeamWaves waves per QP
  // (cmpc_team.hip), on the caller's stream
  int team_grid = 0;    // workgroups resident at two per CU (solve_team_kernel<W, 2>)
  int team_grid1 = 0;   // at one per CU (<W, 1>: B <= CUs)
  size_t team_slab = 0;
  int64_t team_max_batch = -1;  // -1: automatic (B <= 4 x CUs: at most one wave per SIMD)
  // batches of B >= heavy_first_min_batch submit the NC >= 160 class first
  int64_t heavy_first_min_batch = -1;  // -1: automatic (B > 16 x CUs), 0: never
  // The solve kernels (cmpc_wave.hip solve_group_kernel: the NC <= 128 class, the NC 144 / 160
  // class, the NC 192 bin) run concurrently: one class on the caller's stream, the other on a
  // plan stream, the NC 192 kernel on a second plan stream, both forked from / joined to the
  // caller's.  Three streams in total stay within the device's hardware queues
  // (GPU_MAX_HW_QUEUES = 4), so the kernels overlap instead of sharing a queue.
  hipStream_t side = nullptr;
  hipStream_t top = nullptr;
  hipEvent_t fork = nullptr;
  hipEvent_t join = nullptr;
  hipEvent_t join_top = nullptr;
  // timing hooks
  bool timing = false;
  struct Rec { hipEvent_t a, b; int group; };
  std::vector<Rec> recs;       // recorded (pending) pairs
  std::vector<Rec> pool;       // free event pairs
};

namespace {
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  return fail(CMPC_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

using KernelFn = void (*)(cmpc::KParams, cmpc::Inputs, cmpc::Outputs, const int*, const int*,
                          const int*, int*, int, float*, size_t);
using TeamFn = void (*)(cmpc::KParams, cmpc::Inputs, cmpc::Outputs, const int*, int64_t,
                        const int*, int*, float*, size_t);

// The plan's workspace, streams and events belong to the device current at cmpc_plan_create:
// every launch must run there (the Python layer makes the tensors' device current).
int check_device(const cmpc_plan* pl, const char* what) {
  int dev = -1;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
  if (dev != pl->device)
    return fail(CMPC_E_INVALID, std::string(what) + ": the current device is not the plan's device");
  return CMPC_OK;
}

// group 0: bins 1 (NC 128) then 0 (NC 96), two waves per SIMD; group 1: bins 3 (NC 160) then
// 2 (NC 144), one wave per SIMD; group 2: bin 4 (NC 192) alone, one wave per SIMD.  qa = the
// group's first (larger) bin.
int group_first_bin(int k) { return k == 0 ? 1 : (k == 1 ? 3 : 4); }

constexpr int kTeamWaves = 4;

KernelFn group_fn(int k) {
  return k == 0 ? cmpc::solve_group_kernel<128, 96>
                : (k == 1 ? cmpc::solve_group_kernel<160, 144> : cmpc::solve_group_kernel<192, 0>);
}

const char* group_name(int k) {
  static const char* names[kNumGroups] = {"solve_group_kernel<128, 96>",
                                          "solve_group_kernel<160, 144>",
                                          "solve_group_kernel<192, 0>"};
  return names[k];
}

// park slab per wave (floats): the one-wave inverse
size_t group_slab(int k) {
  return k == 0 ? std::max(cmpc::Cfg<128>::SLAB, cmpc::Cfg<96>::SLAB)
                : (k == 1 ? std::max(cmpc::Cfg<160>::SLAB, cmpc::Cfg<144>::SLAB) : cmpc::Cfg<192>::SLAB);
}

// which solve kernels a horizon can need: the NC >= 144 class once the horizon can hold more
// than 128 free forces, the NC 192 kernel once more than 160
bool has_group(const cmpc_plan* pl, int k) {
  return k == 0 || cmpc::kBinCap[k == 1 ? 1 : 3] < 12 * pl->kp.N;
}

// The zero-extended copy of a caller's io struct: fields past the caller's size are NULL or 0
// (the structs grow at their end); a size below min_size is not one of the struct's sizes.
// Checked before the plan is touched.
template <class IO>
int io_copy(const IO* io, size_t min_size, const char* what, const char* type, IO& a) {
  if (!io) return fail(CMPC_E_INVALID, std::string(what) + ": null io");
  if (io->size < min_size)
    return fail(CMPC_E_INVALID, std::string(what) + ": io->size is not a " + type + " size");
  memset(&a, 0, sizeof(a));
  memcpy(&a, io, std::min((size_t)io->size, sizeof(a)));
  return CMPC_OK;
}

// The checks of an evaluation entry (cmpc_kkt_io, cmpc_gain_io, cmpc_vjp_io, cmpc_refine_io, cmpc_jvp_io) after io_copy: plan, B, the six
// problem arrays, face_tol, the device.  `own`: the entry's own required arrays are there;
// `between`: the message of a failed check of the entry's own that ranks after the arrays, or NULL.
template <class IO>
int check_problem(const cmpc_plan* pl, int64_t B, const IO& a, bool own, const char* what,
                  const char* between = nullptr) {
  const std::string w(what);
  if (!pl) return fail(CMPC_E_INVALID, w + ": null plan");
  if (B < 1) return fail(CMPC_E_INVALID, w + ": B must be >= 1");
  if (!a.Ad || !a.Bd || !a.gd || !a.x0 || !a.xref || !a.contact || !own)
    return fail(CMPC_E_INVALID, w + ": null array argument");
  if (between) return fail(CMPC_E_INVALID, w + between);
  if (!(a.face_tol >= 0.f) || !std::isfinite(a.face_tol))
    return fail(CMPC_E_INVALID, w + ": face_tol must be finite and >= 0");
  return check_device(pl, what);
}

// the kernels' common argument block from the plan's constants and the io fields
template <class IO>
cmpc::ProblemArgs problem_args(const cmpc_plan* pl, const IO& a) {
  cmpc::ProblemArgs k;
  k.N = pl->kp.N;
  for (int i = 0; i < 12; ++i) {
    k.Q2[i] = pl->kp.Q2[i];
    k.R2[i] = pl->kp.R2[i];
  }
  k.mu = pl->kp.mu;
  k.fz_min = pl->kp.fz_min;
  k.tol = a.face_tol > 0.f ? (double)a.face_tol : 1e-6;
  k.Ad = a.Ad; k.Bd = a.Bd; k.gd = a.gd; k.x0 = a.x0; k.xref = a.xref;
  k.contact = a.contact;
  k.mu_b = a.mu; k.fz_b = a.fz_min; k.Q = a.Q; k.R = a.R;
  return k;
}

// the held-face part of the argument blocks of cmpc_gain_run, cmpc_vjp_run, cmpc_refine_run and
// cmpc_jvp_run:
// given faces take the place of w's unless the kernel reads w for more than its faces (keep_w)
template <class IO>
cmpc::HeldArgs held_args(const cmpc_plan* pl, const IO& a, bool keep_w) {
  return {problem_args(pl, a), a.faces && !keep_w ? nullptr : a.w, a.faces};
}

constexpr const char* kNoFaces = ": w and faces are both null (one must name the held faces)";

// blocks of a grid-stride launch over B items
unsigned grid_stride_blocks(int64_t B, int64_t cap = 8192) {
  return (unsigned)std::min(B, cap);
}

// every kernel launch of this file: `what` names the launch in the error message
template <class K, class... A>
int launch(K kernel, const char* what, unsigned grid, unsigned block, size_t dyn_lds, void* stream,
           A... args) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), dyn_lds, (hipStream_t)stream, args...);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? hip_fail(e, what) : CMPC_OK;
}

// launch an evaluation kernel, one wave per instance, grid-stride over B
template <class K, class... A>
int launch_eval(K kernel, const char* what, int64_t B, size_t dyn_lds, void* stream, A... args) {
  return launch(kernel, what, grid_stride_blocks(B), 64, dyn_lds, stream, args...);
}

// the opening checks of the pipeline entries (dynamics, trajectory, leg controller, plant)
int check_pipeline(const cmpc_plan* pl, const char* what, bool negative,
                   const char* msg = ": negative batch") {
  if (!pl) return fail(CMPC_E_INVALID, std::string(what) + ": null plan");
  if (int rc = check_device(pl, what)) return rc;
  if (negative) return fail(CMPC_E_INVALID, std::string(what) + msg);
  return CMPC_OK;
}

// the checks of the two derivative entries of the dynamics builder after io_copy, in
// cmpc_build_dynamics' order.  `inputs`: its four arrays are there; `missing`: the message of a
// failed check that ranks after them, or NULL.  B == 0 passes (the caller returns before a launch).
int check_dynamics_grad(const cmpc_plan* pl, int64_t B, float dt, bool inputs, const char* missing,
                        const char* what) {
  const std::string w(what);
  if (int rc = check_pipeline(pl, what, B < 0)) return rc;
  if (!(dt > 0.f) || !std::isfinite(dt)) return fail(CMPC_E_INVALID, w + ": dt must be > 0");
  if (B == 0) return CMPC_OK;
  if (!inputs) return fail(CMPC_E_INVALID, w + ": null array argument");
  if (missing) return fail(CMPC_E_INVALID, w + missing);
  return CMPC_OK;
}

// the same for the two derivative entries of the trajectory generator, whose dt is a double
int check_traj_grad(const cmpc_plan* pl, int64_t B, double dt, bool inputs, const char* missing,
                    const char* what) {
  const std::string w(what);
  if (int rc = check_pipeline(pl, what, B < 0)) return rc;
  if (!(dt > 0.0) || !std::isfinite(dt)) return fail(CMPC_E_INVALID, w + ": dt must be > 0");
  if (B == 0) return CMPC_OK;
  if (!inputs) return fail(CMPC_E_INVALID, w + ": null array argument");
  if (missing) return fail(CMPC_E_INVALID, w + missing);
  return CMPC_OK;
}

// the same for the two derivative entries of the plant: cmpc_srb_step's checks, with nsub in
// 1 .. CMPC_SRB_GRAD_MAX_NSUB
template <class IO>
int check_srb_grad(const cmpc_plan* pl, int64_t B, const IO& a, const char* missing,
                   const char* what) {
  const std::string w(what);
  if (int rc = check_pipeline(pl, what, B < 0)) return rc;
  if (a.nsub < 1 || a.nsub > CMPC_SRB_GRAD_MAX_NSUB)
    return fail(CMPC_E_INVALID, w + ": nsub must be in 1 .. " + std::to_string(CMPC_SRB_GRAD_MAX_NSUB));
  if (!(a.dt > 0.0) || !std::isfinite(a.dt)) return fail(CMPC_E_INVALID, w + ": dt must be > 0");
  if (a.force_stride < 12) return fail(CMPC_E_INVALID, w + ": force_stride must be >= 12");
  if (B == 0) return CMPC_OK;
  if (!a.t_now || !a.gait || !a.mass || !a.inertia_body || !a.force || !a.hip || !a.x || !a.feet ||
      !a.contact_state)
    return fail(CMPC_E_INVALID, w + ": null array argument");
  if (missing) return fail(CMPC_E_INVALID, w + missing);
  return CMPC_OK;
}

template <class IO>
cmpc::SrbIn srb_in(const IO& a) {
  return {a.t_now, a.gait, a.mass, a.inertia_body, a.force, a.force_stride, a.hip, a.x, a.feet,
          a.contact_state};
}

}  // namespace

extern "C" {

void cmpc_params_default(cmpc_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->abi_version = CMPC_ABI_VERSION;
  p->N = 16;
  const float Q[12] = {1, 1, 50, 10, 20, 1, 2, 2, 1, 1, 1, 1};  // centroidal_mpc.py:12
  for (int i = 0; i < 12; ++i) {
    p->Q[i] = Q[i];
    p->R[i] = 1e-5f;  // centroidal_mpc.py:13
  }
  p->mu = 0.8f;        // centroidal_mpc.py:15
  p->fz_min = 10.f;    // centroidal_mpc.py:127
  p->eps_abs = 1e-4f;  // centroidal_mpc.py:25-26
  p->eps_rel = 1e-4f;
  p->max_iter = 1000;  // centroidal_mpc.py:27
  p->rho = 1e-4f;
  p->sigma = 1e-6f;    // OSQP default
  p->alpha = 1.6f;     // OSQP default
  p->adaptive_rho_interval = 25;  // centroidal_mpc.py:32
  p->polish_stable = 3;
  p->polish_refine = 2;  // (round 6: 4 -> 2 with the LDL' solve; profiles/r06d_*)
  p->polish_tol = 1e-5f;
  p->polish_repairs = 6;
  p->reserved0 = 0;
  p->check_termination = 1;  // (reference OPTS: 10, accepted; see include/cmpc.h)
  p->max_batch = 65536;
}

int cmpc_plan_create(const cmpc_params* p, cmpc_plan** out) {
  if (!p || !out) return fail(CMPC_E_INVALID, "cmpc_plan_create: null argument");
  *out = nullptr;
  if (p->abi_version != CMPC_ABI_VERSION)
    return fail(CMPC_E_INVALID, "cmpc_plan_create: abi_version mismatch");
  if (p->N < 1 || p->N > 16) return fail(CMPC_E_INVALID, "cmpc_plan_create: N must be in 1..16");
  for (int i = 0; i < 12; ++i) {
    if (!(p->Q[i] >= 0.f) || !std::isfinite(p->Q[i]))
      return fail(CMPC_E_INVALID, "cmpc_plan_create: Q must be finite and >= 0");
    if (!(p->R[i] > 0.f) || !std::isfinite(p->R[i]))
      return fail(CMPC_E_INVALID, "cmpc_plan_create: R must be finite and > 0");
  }
  if (!(p->mu > 0.f) || !std::isfinite(p->mu)) return fail(CMPC_E_INVALID, "cmpc_plan_create: mu must be > 0");
  if (!std::isfinite(p->fz_min)) return fail(CMPC_E_INVALID, "cmpc_plan_create: fz_min must be finite");
  if (p->max_iter < 1) return fail(CMPC_E_INVALID, "cmpc_plan_create: max_iter must be >= 1");
  if (!(p->eps_abs >= 0.f) || !std::isfinite(p->eps_abs) || !(p->eps_rel >= 0.f) ||
      !std::isfinite(p->eps_rel))
    return fail(CMPC_E_INVALID, "cmpc_plan_create: eps_abs and eps_rel must be finite and >= 0");
  if (!(p->rho > 0.f) || !(p->sigma >= 0.f) || !(p->alpha > 0.f && p->alpha < 2.f))
    return fail(CMPC_E_INVALID, "cmpc_plan_create: need rho > 0, sigma >= 0, 0 < alpha < 2");
  if (p->polish_stable < 1 || p->polish_refine < 1 || !(p->polish_tol > 0.f) ||
      p->polish_repairs < 0 || p->check_termination < 1)
    return fail(CMPC_E_INVALID, "cmpc_plan_create: polish settings out of range");
  if (p->adaptive_rho_interval < 0 || p->max_batch < 1 || p->max_batch > (1LL << 30))
    return fail(CMPC_E_INVALID, "cmpc_plan_create: adaptive_rho_interval/max_batch out of range");
  if (p->reserved0 != 0)
    return fail(CMPC_E_INVALID, "cmpc_plan_create: reserved0 must be 0 (ABI 4's ipm_facts: the "
                                "interior-point fallback was removed)");

  cmpc_plan* pl = new cmpc_plan();
  pl->p = *p;
  cmpc::KParams& k = pl->kp;
  k.N = p->N;
  k.r2_min = 2.f * p->R[0];
  for (int i = 0; i < 12; ++i) {
    k.Q2[i] = 2.f * p->Q[i];
    k.R2[i] = 2.f * p->R[i];
    k.r2_min = std::min(k.r2_min, k.R2[i]);
  }
  k.mu = p->mu;
  k.fz_min = p->fz_min;
  k.rho0 = p->rho;
  k.sigma = p->sigma;
  k.alpha = p->alpha;
  k.eps_abs = p->eps_abs;
  k.eps_rel = p->eps_rel;
  k.polish_tol = p->polish_tol;
  k.max_iter = p->max_iter;
  k.adaptive_interval = p->adaptive_rho_interval;
  k.polish_stable = p->polish_stable;
  k.polish_refine = p->polish_refine;
  k.polish_repairs = p->polish_repairs;
  k.check_every = p->check_termination;

  // every failure from here on: destroy what exists so far (cmpc_plan_destroy tolerates nulls),
  // then set the message
  const auto give_up = [pl](int code, const std::string& msg) {
    cmpc_plan_destroy(pl);
    return fail(code, msg);
  };
  const auto hip_give_up = [&](hipError_t err, const char* what) {
    return give_up(CMPC_E_HIP, std::string(what) + ": " + hipGetErrorString(err));
  };
  hipError_t e = hipGetDevice(&pl->device);
  if (e != hipSuccess) return hip_give_up(e, "hipGetDevice");
  int cus = 0;
  e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, pl->device);
  pl->cus = cus;
  if (e != hipSuccess) return hip_give_up(e, "hipDeviceGetAttribute");
  // persistent grids: resident workgroups per CU x CUs
  size_t work_floats = 0;
  for (int k = 0; k < kNumGroups; ++k) {
    int nb = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, group_fn(k), 64, 0);
    if (e != hipSuccess) return hip_give_up(e, "hipOccupancyMaxActiveBlocksPerMultiprocessor");
    if (nb < 1) return give_up(CMPC_E_HIP, "cmpc_plan_create: solve kernel cannot be resident");
#ifdef CMPC_STAMPS
    if (const char* cap = getenv("CMPC_BLOCKS_PER_CU")) {  // diagnostic build: occupancy sweep
      const int c = atoi(cap);
      if (c >= 1 && c < nb) nb = c;
    }
#endif
    pl->grid[k] = nb * cus;
    pl->slab[k] = group_slab(k);
    pl->work_off[k] = work_floats;
    work_floats += (size_t)pl->grid[k] * pl->slab[k];
  }
  {
    int nb = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, cmpc::solve_team_kernel<kTeamWaves, 2>,
                                                     64 * kTeamWaves, 0);
    if (e != hipSuccess) return hip_give_up(e, "hipOccupancyMaxActiveBlocksPerMultiprocessor");
    if (nb < 1) nb = 1;
    pl->team_grid = nb * cus;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, cmpc::solve_team_kernel<kTeamWaves, 1>,
                                                     64 * kTeamWaves, 0);
    if (e != hipSuccess) return hip_give_up(e, "hipOccupancyMaxActiveBlocksPerMultiprocessor");
    // (0 if the one-per-CU image cannot be resident: team_one_per_cu then never selects it and
    // the two-per-CU image serves every team batch)
    pl->team_grid1 = nb < 1 ? 0 : cus;
    pl->team_slab = std::max({cmpc::TeamCfg<192, kTeamWaves>::SLAB, cmpc::TeamCfg<160, kTeamWaves>::SLAB,
                              cmpc::TeamCfg<128, kTeamWaves>::SLAB, cmpc::TeamCfg<96, kTeamWaves>::SLAB});
    work_floats = std::max(work_floats, (size_t)pl->team_grid * pl->team_slab);
  }
  if (hipMalloc(&pl->d_counters, 2 * cmpc::kNumBins * sizeof(int)) != hipSuccess)
    return give_up(CMPC_E_NOMEM, "hipMalloc counters failed");
  if (hipMalloc(&pl->d_work, work_floats * sizeof(float)) != hipSuccess)
    return give_up(CMPC_E_NOMEM, "hipMalloc workspace failed");
  if (hipMalloc(&pl->d_lists, (size_t)cmpc::kNumBins * p->max_batch * sizeof(int)) != hipSuccess)
    return give_up(CMPC_E_NOMEM, "hipMalloc lists failed");
  if (hipMalloc(&pl->d_stats, CMPC_NUM_STATS * sizeof(unsigned long long)) != hipSuccess)
    return give_up(CMPC_E_NOMEM, "hipMalloc stats failed");
  // the NC 192 stream at the highest priority: its few early waves are dispatched ahead of the
  // register classes submitted right after them on the other queues (solve_impl)
  int prio_lo = 0, prio_hi = 0;
  if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) prio_hi = 0;
  if ((e = hipStreamCreateWithFlags(&pl->side, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipStreamCreateWithPriority(&pl->top, hipStreamNonBlocking, prio_hi)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&pl->fork, hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&pl->join, hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&pl->join_top, hipEventDisableTiming)) != hipSuccess)
    return hip_give_up(e, "side stream/event creation");
  // zeroed on the plan's own stream: a copy or memset on the null stream here (the caller's
  // default stream, round 6's first ABI-6 build) made the closed loop's HIP-graph replay at
  // 65,536 robots 1.3x slower than eager (profiles/r06l_*)
  if ((e = hipMemsetAsync(pl->d_stats, 0, CMPC_NUM_STATS * sizeof(unsigned long long), pl->side)) !=
          hipSuccess ||
      (e = hipStreamSynchronize(pl->side)) != hipSuccess)
    return hip_give_up(e, "hipMemsetAsync stats");
  *out = pl;
  g_err.clear();
  return CMPC_OK;
}

static int solve_impl(cmpc_plan* pl, int64_t B, const cmpc::Inputs& in, const cmpc::Outputs& out,
                      void* stream);

// Every solve entry ends here with its arguments in a cmpc_solve_io (`what` names the entry in
// the messages): the checks, then the kernels' Inputs / Outputs.
static int solve_io(cmpc_plan* pl, int64_t B, const cmpc_solve_io& a, void* stream,
                    const char* what) {
  const std::string w(what);
  if (!pl) return fail(CMPC_E_INVALID, w + ": null plan");
  if (B < 0) return fail(CMPC_E_INVALID, w + ": negative batch");
  if (B == 0) return CMPC_OK;
  if (B > pl->p.max_batch) return fail(CMPC_E_RANGE, w + ": B exceeds plan max_batch");
  if (!a.Ad || !a.Bd || !a.gd || !a.x0 || !a.xref || !a.contact || !a.w_out || !a.status ||
      !a.iters)
    return fail(CMPC_E_INVALID, w + ": null array argument");
  cmpc::Inputs in;
  in.Ad = a.Ad; in.Bd = a.Bd; in.gd = a.gd; in.x0 = a.x0; in.xref = a.xref;
  in.contact = a.contact;
  in.w_init = a.w_init; in.y_init = a.y_init; in.lam_init = a.lam_init;
  in.mu = a.mu; in.fz_min = a.fz_min; in.Q = a.Q; in.R = a.R;
  cmpc::Outputs out;
  out.w = a.w_out; out.status = a.status; out.iters = a.iters;
  out.y = a.y_out; out.lam = a.lam_out;
  out.stats = pl->d_stats;
  return solve_impl(pl, B, in, out, stream);
}

// the arguments every positional solve entry takes, as a cmpc_solve_io with the rest NULL
static cmpc_solve_io positional_io(const float* Ad, const float* Bd, const float* gd,
                                   const float* x0, const float* xref, const uint8_t* contact,
                                   const float* w_init, float* w_out, int32_t* status,
                                   int32_t* iters) {
  cmpc_solve_io a;
  memset(&a, 0, sizeof(a));
  a.size = sizeof(a);
  a.Ad = Ad; a.Bd = Bd; a.gd = gd; a.x0 = x0; a.xref = xref; a.contact = contact;
  a.w_init = w_init; a.w_out = w_out; a.status = status; a.iters = iters;
  return a;
}

int cmpc_solve(cmpc_plan* pl, int64_t B, const float* Ad, const float* Bd, const float* gd,
               const float* x0, const float* xref, const uint8_t* contact, float* w_out,
               int32_t* status, int32_t* iters, void* stream) {
  return solve_io(pl, B, positional_io(Ad, Bd, gd, x0, xref, contact, nullptr, w_out, status, iters),
                  stream, "cmpc_solve");
}

int cmpc_solve_warm(cmpc_plan* pl, int64_t B, const float* Ad, const float* Bd,
                    const float* gd, const float* x0, const float* xref,
                    const uint8_t* contact, const float* w_init, const float* y_init,
                    float* w_out, float* y_out, int32_t* status, int32_t* iters, void* stream) {
  cmpc_solve_io a = positional_io(Ad, Bd, gd, x0, xref, contact, w_init, w_out, status, iters);
  a.y_init = y_init;
  a.y_out = y_out;
  return solve_io(pl, B, a, stream, "cmpc_solve_warm");
}

int cmpc_solve_ref(cmpc_plan* pl, int64_t B, const float* Ad, const float* Bd, const float* gd,
                   const float* x0, const float* xref, const uint8_t* contact,
                   const float* w_init, const float* lam_init, float* w_out, float* lam_out,
                   int32_t* status, int32_t* iters, void* stream) {
  cmpc_solve_io a = positional_io(Ad, Bd, gd, x0, xref, contact, w_init, w_out, status, iters);
  a.lam_init = lam_init;
  a.lam_out = lam_out;
  return solve_io(pl, B, a, stream, "cmpc_solve_ref");
}

int cmpc_solve_io_run(cmpc_plan* pl, int64_t B, const cmpc_solve_io* io, void* stream) {
  cmpc_solve_io a;
  if (int rc = io_copy(io, offsetof(cmpc_solve_io, Ad), "cmpc_solve_io_run", "cmpc_solve_io", a))
    return rc;
  if ((a.y_init || a.y_out) && (a.lam_init || a.lam_out))
    return fail(CMPC_E_INVALID, "cmpc_solve_io_run: y_init / y_out (this solver's dual) and "
                                "lam_init / lam_out (the reference's multipliers) are exclusive");
  return solve_io(pl, B, a, stream, "cmpc_solve_io_run");
}

int cmpc_kkt_run(cmpc_plan* pl, int64_t B, const cmpc_kkt_io* io, void* stream) {
  cmpc_kkt_io a;
  if (int rc = io_copy(io, offsetof(cmpc_kkt_io, res) + sizeof(io->res), "cmpc_kkt_run",
                       "cmpc_kkt_io", a))
    return rc;
  if (int rc = check_problem(pl, B, a, a.w && a.res, "cmpc_kkt_run")) return rc;
  const cmpc::KktArgs k{problem_args(pl, a), a.w, a.lam, a.res};
  return launch_eval(cmpc::kkt_kernel, "kkt_kernel launch", B, 0, stream, k, B);
}

int cmpc_gain_run(cmpc_plan* pl, int64_t B, const cmpc_gain_io* io, void* stream) {
  cmpc_gain_io a;
  if (int rc = io_copy(io, offsetof(cmpc_gain_io, K) + sizeof(io->K), "cmpc_gain_run",
                       "cmpc_gain_io", a))
    return rc;
  if (int rc = check_problem(pl, B, a, a.K, "cmpc_gain_run", a.w || a.faces ? nullptr : kNoFaces))
    return rc;
  const cmpc::GainArgs k{held_args(pl, a, false), a.K, a.Vx, a.Vxx, a.u_star, a.faces_out};
  // the forward pass needs every step's (K_k, kappa_k) in LDS; K alone keeps one slot
  const int keep = a.u_star ? 1 : 0;
  const size_t dyn = (size_t)(keep ? k.p.N : 1) * cmpc::kGainSlot * sizeof(double);
  return launch_eval(cmpc::gain_kernel, "gain_kernel launch", B, dyn, stream, k, B, keep);
}

int cmpc_vjp_run(cmpc_plan* pl, int64_t B, const cmpc_vjp_io* io, void* stream) {
  cmpc_vjp_io a;
  if (int rc = io_copy(io, offsetof(cmpc_vjp_io, g_x0) + sizeof(io->g_x0), "cmpc_vjp_run",
                       "cmpc_vjp_io", a))
    return rc;
  const bool any = a.g_x0 || a.g_xref || a.g_gd || a.g_Q || a.g_R || a.g_mu || a.g_fz_min ||
                   a.g_Ad || a.g_Bd;
  if (int rc = check_problem(pl, B, a, a.gw, "cmpc_vjp_run",
                             !(a.w || a.faces) ? kNoFaces
                             : !any ? ": every output is null (one must be given)" : nullptr))
    return rc;
  const cmpc::VjpArgs k{held_args(pl, a, false), a.gw, a.g_x0, a.g_xref, a.g_gd, a.g_Q, a.g_R,
                        a.g_mu, a.g_fz_min, a.g_Ad, a.g_Bd};
  const size_t dyn = (size_t)k.p.N * cmpc::kVjpSlot * sizeof(double);
  return launch_eval(cmpc::vjp_kernel, "vjp_kernel launch", B, dyn, stream, k, B);
}

int cmpc_jvp_run(cmpc_plan* pl, int64_t B, const cmpc_jvp_io* io, void* stream) {
  cmpc_jvp_io a;
  if (int rc = io_copy(io, offsetof(cmpc_jvp_io, dw) + sizeof(io->dw), "cmpc_jvp_run",
                       "cmpc_jvp_io", a))
    return rc;
  const bool any = a.d_x0 || a.d_xref || a.d_gd || a.d_Q || a.d_R || a.d_mu || a.d_fz_min ||
                   a.d_Ad || a.d_Bd;
  if (int rc = check_problem(pl, B, a, a.dw, "cmpc_jvp_run",
                             !(a.w || a.faces) ? kNoFaces
                             : !any ? ": every tangent is null (one must be given)" : nullptr))
    return rc;
  const cmpc::JvpArgs k{held_args(pl, a, false), a.d_x0, a.d_xref, a.d_gd, a.d_Q, a.d_R,
                        a.d_mu, a.d_fz_min, a.d_Ad, a.d_Bd, a.dw};
  const size_t dyn = (size_t)k.p.N * cmpc::kGainSlot * sizeof(double);  // every step's (K_k, kappa_k)
  return launch_eval(cmpc::jvp_kernel, "jvp_kernel launch", B, dyn, stream, k, B);
}

int cmpc_refine_run(cmpc_plan* pl, int64_t B, const cmpc_refine_io* io, void* stream) {
  cmpc_refine_io a;
  if (int rc = io_copy(io, offsetof(cmpc_refine_io, info) + sizeof(io->info), "cmpc_refine_run",
                       "cmpc_refine_io", a))
    return rc;
  const auto tol_ok = [](float t) { return t >= 0.f && std::isfinite(t); };
  if (int rc = check_problem(
          pl, B, a, a.info, "cmpc_refine_run",
          !(a.w || a.faces) ? kNoFaces
          : a.max_rounds < 0 || a.max_rounds > CMPC_REFINE_MAX_ROUNDS
              ? ": max_rounds must be in 0..16"
          : !tol_ok(a.prim_tol) || !tol_ok(a.dual_tol)
              ? ": prim_tol and dual_tol must be finite and >= 0"
              : nullptr))
    return rc;
  const cmpc::RefineArgs k{held_args(pl, a, true), a.max_rounds,
                           a.prim_tol > 0.f ? (double)a.prim_tol : 1e-9,
                           a.dual_tol > 0.f ? (double)a.dual_tol : 1e-9,
                           a.info, a.res, a.w64, a.lam_out, a.faces_out, a.w_out, a.status};
  const size_t dyn = (size_t)k.p.N * cmpc::kGainSlot * sizeof(double);  // every step's (K_k, kappa_k)
  return launch_eval(cmpc::refine_kernel, "refine_kernel launch", B, dyn, stream, k, B);
}

// The event pair around one solve-kernel launch (cmpc_plan_timing_read).  timing_begin takes a
// pair from the pool (or creates one) and records `a` on stream s; timing_end records `b` and
// files the pair as pending.  A launch that is not recorded (timing off, `timed` false, or the
// record is full) leaves rec.a null, and timing_end then does nothing.
static int timing_begin(cmpc_plan* pl, int group, hipStream_t s, bool timed, cmpc_plan::Rec& rec) {
  hipError_t e;
  rec = cmpc_plan::Rec{nullptr, nullptr, group};
  if (!(timed && pl->timing && pl->recs.size() < 4096 * kNumGroups)) return CMPC_OK;
  if (!pl->pool.empty()) {
    rec = pl->pool.back();
    pl->pool.pop_back();
    rec.group = group;
  } else {
    cmpc_plan::Rec fresh{nullptr, nullptr, group};
    if ((e = hipEventCreate(&fresh.a)) != hipSuccess) return hip_fail(e, "hipEventCreate");
    if ((e = hipEventCreate(&fresh.b)) != hipSuccess) return hip_fail(e, "hipEventCreate");
    rec = fresh;
  }
  if ((e = hipEventRecord(rec.a, s)) != hipSuccess) return hip_fail(e, "hipEventRecord");
  return CMPC_OK;
}

static int timing_end(cmpc_plan* pl, hipStream_t s, const cmpc_plan::Rec& rec) {
  if (!rec.a) return CMPC_OK;
  const hipError_t e = hipEventRecord(rec.b, s);
  if (e != hipSuccess) return hip_fail(e, "hipEventRecord");
  pl->recs.push_back(rec);
  return CMPC_OK;
}

// group k's persistent kernel with g waves whose park slabs start at wave w0 of the group's
// region (a second launch of the same group on the same queue heads takes the slabs after the
// first one's); `timed` records the launch for cmpc_plan_timing_read
static int record_launch(cmpc_plan* pl, int k, hipStream_t s, const cmpc::KParams& kp,
                         const cmpc::Inputs& in, const cmpc::Outputs& out, unsigned g,
                         unsigned w0 = 0, bool timed = true) {
  cmpc_plan::Rec rec;
  int rc = timing_begin(pl, k, s, timed, rec);
  if (rc != CMPC_OK) return rc;
  const int qa = group_first_bin(k);
  rc = launch(group_fn(k), "solve_group_kernel launch", g, 64, 0, s, kp, in, out,
              pl->d_lists + (size_t)qa * pl->p.max_batch,
              pl->d_lists + (size_t)(qa - 1) * pl->p.max_batch, pl->d_counters,
              pl->d_counters + cmpc::kNumBins, qa,
              pl->d_work + pl->work_off[k] + (size_t)w0 * pl->slab[k], pl->slab[k]);
  return rc != CMPC_OK ? rc : timing_end(pl, s, rec);
}

static int64_t heavy_first_batch(const cmpc_plan* pl) {
  // (0 = never: also when the horizon is too short for an NC >= 144 class to exist)
  if (!has_group(pl, 1)) return 0;
  return pl->heavy_first_min_batch >= 0 ? pl->heavy_first_min_batch : 16LL * pl->cus + 1;
}

static int64_t team_batch(const cmpc_plan* pl) {
  return pl->team_max_batch >= 0 ? pl->team_max_batch : 4LL * pl->cus;
}

// B <= CUs: every QP has a CU of its own, so the team kernel built for one workgroup per CU
// runs (CMPC_TEAM_OCC=2 forces the two-per-CU image, for A/B)
static bool team_one_per_cu(const cmpc_plan* pl, int64_t B) {
  static const int occ = [] {
    const char* v = getenv("CMPC_TEAM_OCC");
    return v ? atoi(v) : 0;
  }();
  // (experiment knob CMPC_TEAM_OCC: 2 = always the two-per-CU image, 1 = always one per CU,
  // persistent over B / CUs instances per workgroup)
  return occ != 2 && pl->team_grid1 > 0 && (occ == 1 || B <= pl->team_grid1);
}

// team mode: one launch for every bin; timed as solve kernel 0 (kernel 1 records no call)
static int record_team_launch(cmpc_plan* pl, hipStream_t s, const cmpc::KParams& kp,
                              const cmpc::Inputs& in, const cmpc::Outputs& out, int64_t B) {
  cmpc_plan::Rec rec;
  int rc = timing_begin(pl, 0, s, true, rec);
  if (rc != CMPC_OK) return rc;
  // one QP per CU: the one-workgroup-per-CU image (512 registers per lane, no spills)
  const bool one = team_one_per_cu(pl, B);
  const TeamFn fn = one ? cmpc::solve_team_kernel<kTeamWaves, 1> : cmpc::solve_team_kernel<kTeamWaves, 2>;
  const int grid = one ? pl->team_grid1 : pl->team_grid;
  rc = launch(fn, "solve_team_kernel launch", (unsigned)(grid < B ? grid : B), 64 * kTeamWaves, 0, s,
              kp, in, out, pl->d_lists, (int64_t)pl->p.max_batch, pl->d_counters,
              pl->d_counters + cmpc::kNumBins, pl->d_work, pl->team_slab);
  return rc != CMPC_OK ? rc : timing_end(pl, s, rec);
}

static int solve_impl(cmpc_plan* pl, int64_t B, const cmpc::Inputs& in, const cmpc::Outputs& out,
                      void* stream) {
  int rc = check_device(pl, "cmpc_solve");
  if (rc != CMPC_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e;
  cmpc::KParams kp = pl->kp;
  // at most one wave per SIMD: latency-bound, the condensation with fewer MFMAs wins
  kp.latency_mode = (B <= 4LL * pl->cus) ? 1 : 0;
  if (B <= 1024) {  // one workgroup bins the batch and zeroes the queue heads (no memset)
    rc = launch(cmpc::bin_small_kernel, "bin_small_kernel launch", 1, 1024, 0, st, pl->kp.N, (int)B,
                in.contact, pl->d_counters, pl->d_counters + cmpc::kNumBins, pl->d_lists,
                pl->p.max_batch);
    if (rc != CMPC_OK) return rc;
  } else {
    e = hipMemsetAsync(pl->d_counters, 0, 2 * cmpc::kNumBins * sizeof(int), st);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    const int threads = 256;
    const unsigned blocks = (unsigned)((B + threads - 1) / threads);
    rc = launch(cmpc::bin_kernel, "bin_kernel launch", blocks, threads, 0, st, pl->kp.N, B,
                in.contact, pl->d_counters, pl->d_lists, pl->p.max_batch);
    if (rc != CMPC_OK) return rc;
  }
  // small batches: a team of kTeamWaves waves per QP, all bins in one kernel on the caller's
  // stream (measured faster than one wave per QP up to B = 4 x CUs on configs 1-3, slower from
  // 2,048 up: DESIGN.md 4g)
  if (B <= team_batch(pl)) return record_team_launch(pl, st, kp, in, out, B);
  // The two classes run concurrently: the class submitted first on the caller's stream, the
  // other (the NC >= 160 class exists only when a step can hold more than 128 / 12 stance legs)
  // on the plan stream, forked after the binning and joined back.  Whichever is submitted first
  // fills the device (two NC <= 128 waves or one NC >= 160 wave per SIMD) and the other takes
  // SIMDs as they free up, so the classes run almost one after the other and the end of the
  // step is the tail of the class that runs last (tools/shard_anatomy.py timelines).  Large
  // batches put the NC >= 160 class first: its tail (one wave per SIMD, ~11 instances per wave)
  // is then filled by NC <= 128 waves, and the NC <= 128 tail (~26 cheaper instances per wave)
  // ends the step -- config 3 at 65,536 12.2 -> 11.8 ms, at 16,384 5.5 -> 4.2 ms; small ones
  // (config 2 at 4,096: 2.0 vs 2.4 ms) keep the NC <= 128 class first.  Heavy-first relies on
  // the LDS slot padding of solve_group_kernel (cmpc_wave.hip kLdsSlot): without it the
  // NC <= 128 waves that replace the NC >= 160 ones fit ~6 instead of 8 per CU.
  // The NC 192 bin (rare: one instance in config 3's 65,536, but every instance of a standing
  // batch) has its own kernel in two launches on the same queue: a few waves (one per 4 CUs)
  // on the second plan stream, submitted before the classes so that they are dispatched before
  // the classes fill the SIMDs and the bin's instances start at the beginning of the step (a
  // one-wave-per-SIMD wave could not start later, with the SIMDs held by two-wave NC <= 128
  // waves); then the rest of the grid on the caller's stream once both classes are done, to
  // drain what the few waves have not taken.  An empty bin costs one dispatch of waves that
  // exit at once on an idle device, instead of 1,024 whole-SIMD waves that trickle in as the
  // classes free their SIMDs (a 5 ms span with 0 instances, round 4).
  const bool big = has_group(pl, 1), top = has_group(pl, 2);
  if (big) {
    if ((e = hipEventRecord(pl->fork, st)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    if ((e = hipStreamWaitEvent(pl->side, pl->fork, 0)) != hipSuccess)
      return hip_fail(e, "hipStreamWaitEvent");
    if (top && (e = hipStreamWaitEvent(pl->top, pl->fork, 0)) != hipSuccess)
      return hip_fail(e, "hipStreamWaitEvent");
  }
  unsigned gk[kNumGroups];
  for (int k = 0; k < kNumGroups; ++k) gk[k] = (unsigned)(pl->grid[k] < B ? pl->grid[k] : B);
  const unsigned top_early = std::min(gk[2], (unsigned)std::max(1, pl->cus / 4));
  if (top) {
    rc = record_launch(pl, 2, pl->top, kp, in, out, top_early);
    if (rc != CMPC_OK) return rc;
  }
  const int64_t hmin = heavy_first_batch(pl);
  const int first = (big && hmin > 0 && B >= hmin) ? 1 : 0;  // class submitted first
  rc = record_launch(pl, first, st, kp, in, out, gk[first]);
  if (rc != CMPC_OK) return rc;
  if (big) {
    rc = record_launch(pl, 1 - first, pl->side, kp, in, out, gk[1 - first]);
    if (rc != CMPC_OK) return rc;
    if ((e = hipEventRecord(pl->join, pl->side)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    if ((e = hipStreamWaitEvent(st, pl->join, 0)) != hipSuccess)
      return hip_fail(e, "hipStreamWaitEvent");
    if (top && gk[2] > top_early) {
      rc = record_launch(pl, 2, st, kp, in, out, gk[2] - top_early, top_early, false);
      if (rc != CMPC_OK) return rc;
    }
    if (top) {
      if ((e = hipEventRecord(pl->join_top, pl->top)) != hipSuccess) return hip_fail(e, "hipEventRecord");
      if ((e = hipStreamWaitEvent(st, pl->join_top, 0)) != hipSuccess)
        return hip_fail(e, "hipStreamWaitEvent");
    }
  }
  return CMPC_OK;
}

int cmpc_build_dynamics(cmpc_plan* pl, int64_t B, float dt, const float* mass,
                        const float* inertia, const float* r_feet, const float* xref, float* Ad,
                        float* Bd, float* gd, void* stream) {
  if (int rc = check_pipeline(pl, "cmpc_build_dynamics", B < 0)) return rc;
  if (!(dt > 0.f) || !std::isfinite(dt)) return fail(CMPC_E_INVALID, "cmpc_build_dynamics: dt must be > 0");
  if (B == 0) return CMPC_OK;
  if (!mass || !inertia || !r_feet || !xref || !Ad || !Bd || !gd)
    return fail(CMPC_E_INVALID, "cmpc_build_dynamics: null array argument");
  // (grid-stride: ~32 resident waves per CU)
  return launch(cmpc::dynamics_kernel, "dynamics_kernel launch", grid_stride_blocks(B), 64, 0, stream,
                pl->kp.N, (double)dt, B, mass, inertia, r_feet, xref, Ad, Bd, gd);
}

int cmpc_dynamics_vjp_run(cmpc_plan* pl, int64_t B, const cmpc_dynamics_vjp_io* io, void* stream) {
  const char* what = "cmpc_dynamics_vjp_run";
  cmpc_dynamics_vjp_io a;
  if (int rc = io_copy(io, offsetof(cmpc_dynamics_vjp_io, g_mass) + sizeof(io->g_mass), what,
                       "cmpc_dynamics_vjp_io", a))
    return rc;
  if (int rc = check_dynamics_grad(
          pl, B, a.dt, a.mass && a.inertia && a.r_feet && a.xref,
          !a.g_Ad && !a.g_Bd ? ": g_Ad and g_Bd are both null (one must be given)"
          : !a.g_mass && !a.g_inertia && !a.g_r_feet && !a.g_yaw
              ? ": every output is null (one must be given)"
              : nullptr,
          what))
    return rc;
  if (B == 0) return CMPC_OK;
  const cmpc::DynVjpArgs k{a.mass, a.inertia, a.r_feet, a.xref, a.g_Ad, a.g_Bd,
                           a.g_mass, a.g_inertia, a.g_r_feet, a.g_yaw};
  return launch(cmpc::vjp_dynamics_kernel, "vjp_dynamics_kernel launch", grid_stride_blocks(B), 64,
                0, stream, pl->kp.N, (double)a.dt, B, k);
}

int cmpc_dynamics_jvp_run(cmpc_plan* pl, int64_t B, const cmpc_dynamics_jvp_io* io, void* stream) {
  const char* what = "cmpc_dynamics_jvp_run";
  cmpc_dynamics_jvp_io a;
  if (int rc = io_copy(io, offsetof(cmpc_dynamics_jvp_io, d_Ad) + sizeof(io->d_Ad), what,
                       "cmpc_dynamics_jvp_io", a))
    return rc;
  if (int rc = check_dynamics_grad(
          pl, B, a.dt, a.mass && a.inertia && a.r_feet && a.xref,
          !a.d_mass && !a.d_inertia && !a.d_r_feet && !a.d_xref
              ? ": every tangent is null (one must be given)"
          : !a.d_Ad && !a.d_Bd ? ": d_Ad and d_Bd are both null (one must be given)" : nullptr,
          what))
    return rc;
  if (B == 0) return CMPC_OK;
  const cmpc::DynJvpArgs k{a.mass, a.inertia, a.r_feet, a.xref, a.d_mass, a.d_inertia,
                           a.d_r_feet, a.d_xref, a.d_Ad, a.d_Bd};
  return launch(cmpc::jvp_dynamics_kernel, "jvp_dynamics_kernel launch", grid_stride_blocks(B), 64,
                0, stream, pl->kp.N, (double)a.dt, B, k);
}

int cmpc_generate_traj(cmpc_plan* pl, int64_t B, double dt, const float* x0, double* pos_des,
                       const float* cmd, const double* t_now, const double* gait,
                       const float* foot_lever, const float* hip, float* xref, uint8_t* contact,
                       float* r_feet, void* stream) {
  if (int rc = check_pipeline(pl, "cmpc_generate_traj", B < 0)) return rc;
  if (!(dt > 0.0) || !std::isfinite(dt)) return fail(CMPC_E_INVALID, "cmpc_generate_traj: dt must be > 0");
  if (B == 0) return CMPC_OK;
  if (!x0 || !pos_des || !cmd || !t_now || !gait || !foot_lever || !hip || !xref || !contact ||
      !r_feet)
    return fail(CMPC_E_INVALID, "cmpc_generate_traj: null array argument");
  // one wave per group of cmpc::kTrajGroup robots (grid-stride over groups)
  const unsigned blocks = grid_stride_blocks((B + cmpc::kTrajGroup - 1) / cmpc::kTrajGroup);
  return launch(cmpc::traj_group_kernel, "traj_group_kernel launch", blocks, 64, 0, stream, pl->kp.N,
                dt, B, x0, pos_des, cmd, t_now, gait, foot_lever, hip, xref, contact, r_feet);
}

int cmpc_traj_vjp_run(cmpc_plan* pl, int64_t B, const cmpc_traj_vjp_io* io, void* stream) {
  const char* what = "cmpc_traj_vjp_run";
  cmpc_traj_vjp_io a;
  if (int rc = io_copy(io, offsetof(cmpc_traj_vjp_io, g_x0) + sizeof(io->g_x0), what,
                       "cmpc_traj_vjp_io", a))
    return rc;
  if (int rc = check_traj_grad(
          pl, B, a.dt, a.x0 && a.pos_des && a.cmd && a.t_now && a.gait && a.hip,
          !a.g_xref && !a.g_r_feet && !a.g_yaw && !a.g_pos_des_out
              ? ": every gradient is null (one must be given)"
          : !a.g_x0 && !a.g_pos_des && !a.g_cmd && !a.g_foot_lever
              ? ": every output is null (one must be given)"
              : nullptr,
          what))
    return rc;
  if (B == 0) return CMPC_OK;
  const cmpc::TrajVjpArgs k{{a.x0, a.pos_des, a.cmd, a.t_now, a.gait, a.hip},
                            a.g_xref, a.g_r_feet, a.g_yaw, a.g_pos_des_out,
                            a.g_x0, a.g_pos_des, a.g_cmd, a.g_foot_lever};
  return launch(cmpc::vjp_traj_kernel, "vjp_traj_kernel launch", grid_stride_blocks(B), 64, 0,
                stream, pl->kp.N, a.dt, B, k);
}

int cmpc_traj_jvp_run(cmpc_plan* pl, int64_t B, const cmpc_traj_jvp_io* io, void* stream) {
  const char* what = "cmpc_traj_jvp_run";
  cmpc_traj_jvp_io a;
  if (int rc = io_copy(io, offsetof(cmpc_traj_jvp_io, d_xref) + sizeof(io->d_xref), what,
                       "cmpc_traj_jvp_io", a))
    return rc;
  if (int rc = check_traj_grad(
          pl, B, a.dt, a.x0 && a.pos_des && a.cmd && a.t_now && a.gait && a.hip,
          !a.d_x0 && !a.d_pos_des && !a.d_cmd && !a.d_foot_lever
              ? ": every tangent is null (one must be given)"
          : !a.d_xref && !a.d_r_feet && !a.d_pos_des_out
              ? ": every output is null (one must be given)"
              : nullptr,
          what))
    return rc;
  if (B == 0) return CMPC_OK;
  const cmpc::TrajJvpArgs k{{a.x0, a.pos_des, a.cmd, a.t_now, a.gait, a.hip},
                            a.d_x0, a.d_pos_des, a.d_cmd, a.d_foot_lever,
                            a.d_xref, a.d_r_feet, a.d_pos_des_out};
  return launch(cmpc::jvp_traj_kernel, "jvp_traj_kernel launch", grid_stride_blocks(B), 64, 0,
                stream, pl->kp.N, a.dt, B, k);
}

int cmpc_leg_torque(cmpc_plan* pl, int64_t B, const double* t, const double* gait,
                    const float* force, int64_t force_stride, const double* J_foot,
                    const double* J_full, const double* M, const double* C, const double* g,
                    const double* dq, const double* Jdot_dq, const double* foot_pos,
                    const double* foot_vel, const double* body, const double* hip,
                    double* state, double tau_max, double* tau, void* stream) {
  if (int rc = check_pipeline(pl, "cmpc_leg_torque", B < 0)) return rc;
  if (force_stride < 12) return fail(CMPC_E_INVALID, "cmpc_leg_torque: force_stride must be >= 12");
  if (!std::isfinite(tau_max)) return fail(CMPC_E_INVALID, "cmpc_leg_torque: tau_max must be finite");
  if (B == 0) return CMPC_OK;
  if (!t || !gait || !force || !J_foot || !J_full || !M || !C || !g || !dq || !Jdot_dq ||
      !foot_pos || !foot_vel || !body || !hip || !state || !tau)
    return fail(CMPC_E_INVALID, "cmpc_leg_torque: null array argument");
  cmpc::LegArgs a{t, gait, force, force_stride, J_foot, J_full, M, C, g, dq, Jdot_dq, foot_pos,
                  foot_vel, body, hip, state, tau_max, tau};
  // (one wave per robot)
  return launch(cmpc::leg_kernel, "leg_kernel launch", grid_stride_blocks(B, 16384), 64, 0, stream,
                B, a);
}

int cmpc_srb_step(cmpc_plan* pl, int64_t B, int nsub, double dt, const double* t_now,
                  const double* gait, const float* mass, const float* inertia_body,
                  const float* force, int64_t force_stride, const float* hip, float* x,
                  float* feet, uint8_t* contact_state, void* stream) {
  if (int rc = check_pipeline(pl, "cmpc_srb_step", B < 0 || nsub < 0, ": negative batch or nsub"))
    return rc;
  if (!(dt > 0.0) || !std::isfinite(dt)) return fail(CMPC_E_INVALID, "cmpc_srb_step: dt must be > 0");
  if (force_stride < 12) return fail(CMPC_E_INVALID, "cmpc_srb_step: force_stride must be >= 12");
  if (B == 0 || nsub == 0) return CMPC_OK;
  if (!t_now || !gait || !mass || !inertia_body || !force || !hip || !x || !feet || !contact_state)
    return fail(CMPC_E_INVALID, "cmpc_srb_step: null array argument");
  const unsigned blocks = (unsigned)((B + 255) / 256);
  return launch(cmpc::srb_kernel, "srb_kernel launch", blocks, 256, 0, stream, B, nsub, dt, t_now,
                gait, mass, inertia_body, force, force_stride, hip, x, feet, contact_state);
}

int cmpc_srb_vjp_run(cmpc_plan* pl, int64_t B, const cmpc_srb_vjp_io* io, void* stream) {
  const char* what = "cmpc_srb_vjp_run";
  cmpc_srb_vjp_io a;
  if (int rc = io_copy(io, offsetof(cmpc_srb_vjp_io, g_x) + sizeof(io->g_x), what,
                       "cmpc_srb_vjp_io", a))
    return rc;
  if (int rc = check_srb_grad(
          pl, B, a,
          !a.g_x_out && !a.g_feet_out ? ": every gradient is null (one must be given)"
          : !a.g_x && !a.g_feet && !a.g_force && !a.g_mass && !a.g_inertia_body
              ? ": every output is null (one must be given)"
              : nullptr,
          what))
    return rc;
  if (B == 0) return CMPC_OK;
  const cmpc::SrbVjpArgs k{srb_in(a), a.g_x_out, a.g_feet_out,
                           a.g_x, a.g_feet, a.g_force, a.g_mass, a.g_inertia_body};
  // one thread per robot, one wave per block; a short call's tape leaves room for two blocks per CU
  const auto kernel = a.nsub <= cmpc::kSrbShortNsub ? cmpc::srb_vjp_kernel<cmpc::kSrbStoredShort>
                                                    : cmpc::srb_vjp_kernel<cmpc::kSrbStoredMax>;
  return launch(kernel, "srb_vjp_kernel launch", (unsigned)((B + 63) / 64), 64, 0, stream, B,
                (int)a.nsub, a.dt, k);
}

int cmpc_srb_jvp_run(cmpc_plan* pl, int64_t B, const cmpc_srb_jvp_io* io, void* stream) {
  const char* what = "cmpc_srb_jvp_run";
  cmpc_srb_jvp_io a;
  if (int rc = io_copy(io, offsetof(cmpc_srb_jvp_io, d_x_out) + sizeof(io->d_x_out), what,
                       "cmpc_srb_jvp_io", a))
    return rc;
  if (int rc = check_srb_grad(
          pl, B, a,
          !a.d_x && !a.d_feet && !a.d_force && !a.d_mass && !a.d_inertia_body
              ? ": every tangent is null (one must be given)"
          : !a.d_x_out && !a.d_feet_out ? ": every output is null (one must be given)"
                                        : nullptr,
          what))
    return rc;
  if (B == 0) return CMPC_OK;
  const cmpc::SrbJvpArgs k{srb_in(a), a.d_x, a.d_feet, a.d_force, a.d_mass, a.d_inertia_body,
                           a.d_x_out, a.d_feet_out};
  return launch(cmpc::srb_jvp_kernel, "srb_jvp_kernel launch", (unsigned)((B + 63) / 64), 64, 0,
                stream, B, (int)a.nsub, a.dt, k);
}

int cmpc_srb_step_io_run(cmpc_plan* pl, int64_t B, const cmpc_srb_io* io, void* stream) {
  const char* what = "cmpc_srb_step_io_run";
  const std::string w(what);
  cmpc_srb_io a;
  if (int rc = io_copy(io, offsetof(cmpc_srb_io, contact_state) + sizeof(io->contact_state), what,
                       "cmpc_srb_io", a))
    return rc;
  if (int rc = check_pipeline(pl, what, B < 0 || a.nsub < 0, ": negative batch or nsub")) return rc;
  if (!(a.dt > 0.0) || !std::isfinite(a.dt)) return fail(CMPC_E_INVALID, w + ": dt must be > 0");
  if (a.force_stride < 12) return fail(CMPC_E_INVALID, w + ": force_stride must be >= 12");
  if (B == 0 || a.nsub == 0) return CMPC_OK;
  if (!a.t_now || !a.gait || !a.mass || !a.inertia_body || !a.force || !a.hip || !a.x || !a.feet ||
      !a.contact_state)
    return fail(CMPC_E_INVALID, w + ": null array argument");
  if (a.K && (!a.x_solve || !a.contact))
    return fail(CMPC_E_INVALID, w + ": K needs x_solve and contact");
  if ((uintptr_t)a.K % 16) return fail(CMPC_E_INVALID, w + ": K must be 16-byte aligned");
  const unsigned blocks = (unsigned)((B + 255) / 256);
  if (!a.K && !a.wrench && !a.force_out && !a.fb_status)  // the plain plant, bit for bit
    return launch(cmpc::srb_kernel, "srb_kernel launch", blocks, 256, 0, stream, B, (int)a.nsub,
                  a.dt, a.t_now, a.gait, a.mass, a.inertia_body, a.force, a.force_stride, a.hip,
                  a.x, a.feet, a.contact_state);
  const cmpc::SrbFbArgs k{a.t_now, a.gait, a.mass, a.inertia_body, a.force, a.force_stride, a.hip,
                          a.x, a.feet, a.contact_state, a.K, a.x_solve, a.contact, a.mu, a.fz_min,
                          pl->kp.mu, pl->kp.fz_min, pl->kp.N, a.wrench, a.force_out, a.fb_status};
  // one thread per robot, one wave per block; with K the block stages its robots' gains in LDS
  const auto kernel = a.K ? cmpc::srb_feedback_kernel<true> : cmpc::srb_feedback_kernel<false>;
  return launch(kernel, "srb_feedback_kernel launch",
                (unsigned)((B + cmpc::kSrbFbRobots - 1) / cmpc::kSrbFbRobots), cmpc::kSrbFbRobots,
                0, stream, B, (int)a.nsub, a.dt, k);
}

int cmpc_plan_set_timing(cmpc_plan* pl, int enable) {
  if (!pl) return fail(CMPC_E_INVALID, "cmpc_plan_set_timing: null plan");
  pl->timing = enable != 0;
  return CMPC_OK;
}

int cmpc_plan_set_team(cmpc_plan* pl, int64_t max_batch) {
  if (!pl) return fail(CMPC_E_INVALID, "cmpc_plan_set_team: null plan");
  if (max_batch < -1) return fail(CMPC_E_INVALID, "cmpc_plan_set_team: max_batch must be >= -1");
  pl->team_max_batch = max_batch;
  return CMPC_OK;
}

int cmpc_plan_team_batch(const cmpc_plan* pl, int64_t* max_batch) {
  if (!pl || !max_batch) return fail(CMPC_E_INVALID, "cmpc_plan_team_batch: null argument");
  *max_batch = team_batch(pl);
  return CMPC_OK;
}

int cmpc_plan_set_heavy_first(cmpc_plan* pl, int64_t min_batch) {
  if (!pl) return fail(CMPC_E_INVALID, "cmpc_plan_set_heavy_first: null plan");
  if (min_batch < -1) return fail(CMPC_E_INVALID, "cmpc_plan_set_heavy_first: min_batch must be >= -1");
  pl->heavy_first_min_batch = min_batch;
  return CMPC_OK;
}

int cmpc_plan_heavy_first_batch(const cmpc_plan* pl, int64_t* min_batch) {
  if (!pl || !min_batch) return fail(CMPC_E_INVALID, "cmpc_plan_heavy_first_batch: null argument");
  *min_batch = heavy_first_batch(pl);
  return CMPC_OK;
}

const char* cmpc_plan_solve_kernel(const cmpc_plan* pl, int64_t B, int k) {
  if (!pl || B < 1 || k < 0 || k >= kNumGroups) return nullptr;
  if (B <= team_batch(pl))
    return k != 0 ? nullptr : team_one_per_cu(pl, B) ? "solve_team_kernel<4, 1>" : "solve_team_kernel<4, 2>";
  if (!has_group(pl, k)) return nullptr;
  return group_name(k);
}

int cmpc_plan_timing_read(cmpc_plan* pl, float* ms_per_kernel, int32_t* calls_per_kernel) {
  if (!pl || !ms_per_kernel || !calls_per_kernel)
    return fail(CMPC_E_INVALID, "cmpc_plan_timing_read: null argument");
  for (int k = 0; k < kNumGroups; ++k) { ms_per_kernel[k] = 0.f; calls_per_kernel[k] = 0; }
  for (auto& r : pl->recs) {
    hipError_t e = hipEventSynchronize(r.b);
    if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize");
    float ms = 0.f;
    e = hipEventElapsedTime(&ms, r.a, r.b);
    if (e != hipSuccess) return hip_fail(e, "hipEventElapsedTime");
    ms_per_kernel[r.group] += ms;
    calls_per_kernel[r.group] += 1;
    pl->pool.push_back(r);
  }
  pl->recs.clear();
  return CMPC_OK;
}

void cmpc_plan_destroy(cmpc_plan* pl) {
  if (!pl) return;
  for (auto& r : pl->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (auto& r : pl->pool) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  if (pl->side) (void)hipStreamDestroy(pl->side);
  if (pl->top) (void)hipStreamDestroy(pl->top);
  if (pl->fork) (void)hipEventDestroy(pl->fork);
  if (pl->join) (void)hipEventDestroy(pl->join);
  if (pl->join_top) (void)hipEventDestroy(pl->join_top);
  (void)hipFree(pl->d_counters);
  (void)hipFree(pl->d_lists);
  (void)hipFree(pl->d_work);
  if (pl->d_stats) (void)hipFree(pl->d_stats);
  delete pl;
}

int cmpc_plan_stats(cmpc_plan* pl, uint64_t* out, int reset) {
  if (!pl || !out) return fail(CMPC_E_INVALID, "cmpc_plan_stats: null argument");
  if (int rc = check_device(pl, "cmpc_plan_stats")) return rc;
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
  // (on the plan's stream, not the null stream: see cmpc_plan_create)
  unsigned long long v[CMPC_NUM_STATS];
  if ((e = hipMemcpyAsync(v, pl->d_stats, sizeof(v), hipMemcpyDeviceToHost, pl->side)) != hipSuccess ||
      (reset && (e = hipMemsetAsync(pl->d_stats, 0, sizeof(v), pl->side)) != hipSuccess) ||
      (e = hipStreamSynchronize(pl->side)) != hipSuccess)
    return hip_fail(e, "cmpc_plan_stats copy");
  for (int i = 0; i < CMPC_NUM_STATS; ++i) out[i] = (uint64_t)v[i];
  return CMPC_OK;
}

#ifdef CMPC_STAMPS
// diagnostic build only: read and clear the per-phase cycle counters
int cmpc_debug_stamps(unsigned long long* out32) {
  hipError_t e = hipMemcpyFromSymbol(out32, HIP_SYMBOL(cmpc::g_stamps), 32 * sizeof(unsigned long long));
  if (e != hipSuccess) return hip_fail(e, "hipMemcpyFromSymbol");
  unsigned long long z[32] = {0};
  e = hipMemcpyToSymbol(HIP_SYMBOL(cmpc::g_stamps), z, sizeof(z));
  if (e != hipSuccess) return hip_fail(e, "hipMemcpyToSymbol");
  return CMPC_OK;
}
#endif

const char* cmpc_last_error(void) { return g_err.c_str(); }

const char* cmpc_version(void) { return "cmpc 1 gfx950"; }

}  // extern "C"
