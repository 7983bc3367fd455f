// cmpc_diag.h -- the diagnostic builds of the solve kernels, kept out of the product text.
// Included by cmpc_wave_prims.h inside namespace cmpc, after the wave helpers (opaque_lane,
// wave_sum, uniformf, WSYNC).  solve_instance, its phases and polish_check call the hooks of
// one `Diag` object and the trace macros; in a product build every hook is an empty inline
// function, the object has no data and the macros expand to nothing.
//
//   -DCMPC_TRACE=id / -DCMPC_TRACE_IDS=id,id,...  device printf of one instance's (several
//       instances') ADMM iterations, polish sessions, refinements and KKT checks, every line
//       prefixed with the instance index
//   -DCMPC_DIAG_COUNTS   status = cycles / 16, iters = iters | attempts | flags | factorizations,
//                        w[0..7] = cycles and factorizations at failed sessions 1..4
//   -DCMPC_DIAG_GRES     w[0..2] = gradient and face metrics of the accepted point, force scale
//   -DCMPC_DIAG_TIMES    status = start, iters = duration on the 100 MHz constant clock
//   -DCMPC_POISON_LDS / -DCMPC_POISON_PARK   NaN into the float scratch / the wave's park slab
//                        before every instance (W = 1)
// (-DCMPC_STAMPS: the CMPC_T0 / CMPC_ACC / CMPC_CNT one-liners of cmpc_wave_prims.h.)
#pragma once

#if defined(CMPC_TRACE_IDS) && !defined(CMPC_TRACE)
#define CMPC_TRACE (-1)
#endif
#ifdef CMPC_TRACE
__device__ __forceinline__ bool trace_on(int64_t b) {
#ifdef CMPC_TRACE_IDS
  constexpr int64_t ids[] = {CMPC_TRACE_IDS};
  bool on = false;
  for (int64_t i : ids) on |= (b == i);
  return on;
#else
  return b == CMPC_TRACE;
#endif
}
// TRACE_IF: printf on the lanes where `cond` holds.  TRACEF: one line from lane 0 of the traced
// instance (`lane` is the caller's); values that need the whole wave (a reduction, a vote) are
// computed before it, inside `if (trace_on(b)) { ... }`.
#define TRACE_IF(cond, ...) \
  do { if (cond) printf(__VA_ARGS__); } while (0)
#define TRACEF(b, fmt, ...) TRACE_IF(trace_on(b) && lane == 0, "[%d] " fmt, (int)(b), ##__VA_ARGS__)
#else
__device__ __forceinline__ constexpr bool trace_on(int64_t) { return false; }
#define TRACE_IF(cond, ...) (void)0
#define TRACEF(b, fmt, ...) (void)0
#endif
// polish_check's per-triple trace: the instance index where it is traced, else -1
__device__ __forceinline__ int trace_id(int64_t b) { return trace_on(b) ? (int)b : -1; }

struct Diag {
  // flags of the counts build (tools/diag_counts.py)
  static constexpr int kLoose = 1;     // loose acceptance
  static constexpr int kCertMiss = 2;  // certified face bound missed
  static constexpr int kDdStall = 4;   // a check on a stalled downdated refinement redone on a
                                       // fresh factorization
#ifdef CMPC_DIAG_GRES
  float gm = -1.f, cm = -1.f, us = 0.f;  // (-1: not a polished point)
#endif
#ifdef CMPC_DIAG_COUNTS
  int fact = 0, pol = 0, flags = 0;
  unsigned long long t0 = 0;
  float fail_t[4] = {0.f, 0.f, 0.f, 0.f};  // cycles at the end of failed sessions 1..4
  int fail_f[4] = {0, 0, 0, 0};            // factorizations by then
  int nf = 0;
#endif
#ifdef CMPC_DIAG_TIMES  // start / end on the 100 MHz constant clock
  unsigned long long rt0 = 0;
#endif

  // NaN into the float scratch (gbuf: the G slab, vbuf) and / or the wave's park slab
  __device__ __forceinline__ void poison(bool single_wave, float* gbuf, int ng, float* vbuf, int nv,
                                         float* park, int slab, int lane) {
#if defined(CMPC_POISON_LDS)
    if (single_wave) {
      const float qn = __int_as_float(0x7fc00000);
      for (int i = lane; i < ng; i += 64) gbuf[i] = qn;
      for (int i = lane; i < nv; i += 64) vbuf[i] = qn;
      WSYNC();
    }
#endif
#if defined(CMPC_POISON_PARK)
    if (single_wave) {
      const float qn = __int_as_float(0x7fc00000);
      for (int i = lane; i < slab; i += 64) park[i] = qn;
    }
#endif
  }

  // the instance is set up; the iteration starts
  __device__ __forceinline__ void begin() {
#ifdef CMPC_DIAG_COUNTS
    t0 = __builtin_amdgcn_s_memtime();
#endif
#ifdef CMPC_DIAG_TIMES
    rt0 = __builtin_amdgcn_s_memrealtime();
#endif
  }
  __device__ __forceinline__ void factor() {
#ifdef CMPC_DIAG_COUNTS
    ++fact;
#endif
  }
  __device__ __forceinline__ void polish_attempt() {
#ifdef CMPC_DIAG_COUNTS
    ++pol;
#endif
  }
  __device__ __forceinline__ void flag(int bit) {
#ifdef CMPC_DIAG_COUNTS
    flags |= bit;
#endif
  }
  __device__ __forceinline__ void session_failed() {
#ifdef CMPC_DIAG_COUNTS
    if (nf < 4) {
      fail_t[nf] = (float)(__builtin_amdgcn_s_memtime() - t0);
      fail_f[nf] = fact;
    }
    ++nf;
#endif
  }
  // at an accepted point: |grad|_2 (the gradient at the final refinement point, s.g over the nact
  // params) and |c|_2 (polish_check's per-triple |c_t|^2 in s.r), both over min 2R x the force
  // scale (force-error units)
  template <class S>
  __device__ __forceinline__ void accepted(S& s, float r2_min, int nact) {
#ifdef CMPC_DIAG_GRES
    const int lane = opaque_lane();
    WSYNC();
    float g2 = 0.f;
    for (int p = lane; p < nact; p += 64) g2 = fmaf(s.g[p], s.g[p], g2);
    g2 = wave_sum(g2);
    const float c2 = wave_sum(s.r[lane]);
    us = uniformf(s.r[64]);
    gm = uniformf(sqrtf(g2)) / (r2_min * us);
    cm = uniformf(sqrtf(c2)) / (r2_min * us);
#endif
  }
  // status / iters of instance b, and in the counts / gres builds the first floats of its w
  // row (wb): the real values in a product build, else the build's encoding
  __device__ __forceinline__ void finish(int32_t* status_out, int32_t* iters_out, float* wb,
                                         int64_t b, int lane, int status, int iters) {
#ifdef CMPC_DIAG_COUNTS
    if (lane < 4) wb[lane] = fail_t[lane];
    else if (lane < 8) wb[lane] = (float)fail_f[lane - 4];
#endif
#ifdef CMPC_DIAG_GRES
    if (lane == 0) { wb[0] = gm; wb[1] = cm; wb[2] = us; }
#endif
    if (lane == 0) {
#if defined(CMPC_DIAG_COUNTS)  // iters | attempts | flags | factorizations, cycles / 16
      status_out[b] = (int)((__builtin_amdgcn_s_memtime() - t0) >> 4);
      iters_out[b] = iters + 1000 * (pol + 100 * flags) + 1000000 * fact;
#elif defined(CMPC_DIAG_TIMES)  // start (10 ns ticks, low 31 bits) | duration + 1e9 if teamed
      status_out[b] = (int)(rt0 & 0x7fffffffull);
      iters_out[b] = (int)(__builtin_amdgcn_s_memrealtime() - rt0);
#else
      status_out[b] = status;
      iters_out[b] = iters;
#endif
    }
  }
};
