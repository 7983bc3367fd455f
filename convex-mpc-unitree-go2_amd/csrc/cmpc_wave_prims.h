// cmpc_wave_prims.h -- wave primitives of the solve kernels: vector types, DPP / permlane moves,
// wave reductions and scans, the MFMA wrapper, WSYNC and the diagnostic macros.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cmpc {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------
// wave helpers
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float readlane_f(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}

// wave-uniform copy of a value the compiler cannot prove uniform (keeps branches scalar)
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uniformf(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// v[l] and v[l ^ 32] (resp. v[l ^ 16]) without address registers (gfx950 permlane swaps):
// after the swap the two results hold the lane's own value and its partner's in some order
__device__ __forceinline__ void pair32(float v, float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_int(v), __float_as_int(v), false, false);
  a = __int_as_float(r[0]);
  b = __int_as_float(r[1]);
}
__device__ __forceinline__ void pair16(float v, float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_int(v), __float_as_int(v), false, false);
  a = __int_as_float(r[0]);
  b = __int_as_float(r[1]);
}

// max over the wave, result in every lane
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, dpp<0xB1>(v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp<0x4E>(v));   // quad_perm [2,3,0,1]
  v = fmaxf(v, dpp<0x141>(v));  // row_half_mirror
  v = fmaxf(v, dpp<0x140>(v));  // row_mirror
  float a, b;
  pair32(v, a, b);
  v = fmaxf(a, b);
  pair16(v, a, b);
  return fmaxf(a, b);
}

// exclusive prefix sum of small non-negative counts (< 4) across the wave
__device__ __forceinline__ int wave_excl_scan4(int v) {
  const unsigned long long b0 = __ballot(v & 1), b1 = __ballot(v & 2);
  const int c0 = __builtin_amdgcn_mbcnt_hi((unsigned)(b0 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b0, 0));
  const int c1 = __builtin_amdgcn_mbcnt_hi((unsigned)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b1, 0));
  return c0 + 2 * c1;
}
__device__ __forceinline__ int wave_total4(int v) {
  return __popcll(__ballot(v & 1)) + 2 * __popcll(__ballot(v & 2));
}

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

typedef double d4 __attribute__((ext_vector_type(4)));

// 64-bit DPP move (two 32-bit moves; with bound_ctrl a lane past the row reads 0.0)
template <int CTRL>
__device__ __forceinline__ double dpp64(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_mov_dpp((int)(unsigned)(b & 0xffffffffll), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xF, 0xF, true);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// sum over the 16 lanes of a DPP row (lanes with equal lane>>4), result in every lane
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp<0x141>(v);  // row_half_mirror
  v += dpp<0x140>(v);  // row_mirror
  return v;
}

// row16_sum of four values at once, step by step across the four: each chain keeps its own
// order, and no DPP step reads the register written by the instruction before it
__device__ __forceinline__ void row16_sum4(float& a, float& b, float& c, float& d) {
  a += dpp<0xB1>(a), b += dpp<0xB1>(b), c += dpp<0xB1>(c), d += dpp<0xB1>(d);
  a += dpp<0x4E>(a), b += dpp<0x4E>(b), c += dpp<0x4E>(c), d += dpp<0x4E>(d);
  a += dpp<0x141>(a), b += dpp<0x141>(b), c += dpp<0x141>(c), d += dpp<0x141>(d);
  a += dpp<0x140>(a), b += dpp<0x140>(b), c += dpp<0x140>(c), d += dpp<0x140>(d);
}

// shift by D lanes along the DPP row, towards lower lanes (SHL: row_shl, lane c reads c + D) or
// higher ones (row_shr, lane c reads c - D); a lane past the row reads zero
template <bool SHL, int D>
__device__ __forceinline__ float row_shift(float v) { return dpp<(SHL ? 0x100 : 0x110) + D>(v); }
template <bool SHL, int D>
__device__ __forceinline__ double row_shift(double v) { return dpp64<(SHL ? 0x100 : 0x110) + D>(v); }
// the same by 2^l lanes, l = 0 .. 3 (a constant once the caller's loop is unrolled)
template <bool SHL>
__device__ __forceinline__ float row_shift_pow2(float v, int l) {
  switch (l) {
    case 0: return row_shift<SHL, 1>(v);
    case 1: return row_shift<SHL, 2>(v);
    case 2: return row_shift<SHL, 4>(v);
    default: return row_shift<SHL, 8>(v);
  }
}
// x <- its inclusive scan along the row (prefix sums, or suffix sums for SHL), y <- the exclusive
// scan of that scan
template <bool SHL, class T>
__device__ __forceinline__ void row_scan2(T& x, T& y) {
  x += row_shift<SHL, 1>(x);
  x += row_shift<SHL, 2>(x);
  x += row_shift<SHL, 4>(x);
  x += row_shift<SHL, 8>(x);
  y = row_shift<SHL, 1>(x);
  y += row_shift<SHL, 1>(y);
  y += row_shift<SHL, 2>(y);
  y += row_shift<SHL, 4>(y);
  y += row_shift<SHL, 8>(y);
}

// row_scan2 of three values at once, step by step across the three: each chain keeps its own
// order, and no DPP step reads the register written by the instruction before it
template <bool SHL, class T>
__device__ __forceinline__ void row_scan2x3(T (&x)[3], T (&y)[3]) {
#define CMPC_SCAN_STEP(v, D)   \
  _Pragma("unroll") for (int q = 0; q < 3; ++q) v[q] += row_shift<SHL, D>(v[q])
  CMPC_SCAN_STEP(x, 1);
  CMPC_SCAN_STEP(x, 2);
  CMPC_SCAN_STEP(x, 4);
  CMPC_SCAN_STEP(x, 8);
#pragma unroll
  for (int q = 0; q < 3; ++q) y[q] = row_shift<SHL, 1>(x[q]);
  CMPC_SCAN_STEP(y, 1);
  CMPC_SCAN_STEP(y, 2);
  CMPC_SCAN_STEP(y, 4);
  CMPC_SCAN_STEP(y, 8);
#undef CMPC_SCAN_STEP
}

// sum over the 4 rows (lanes c, c+16, c+32, c+48), result in every lane
__device__ __forceinline__ float col4_sum(float v) {
  float a, b;
  pair32(v, a, b);
  pair16(a + b, a, b);
  return a + b;
}

// sum over the wave, result in every lane
__device__ __forceinline__ float wave_sum(float v) { return col4_sum(row16_sum(v)); }

// Lane id the compiler cannot see as loop invariant: every phase re-derives its lane-dependent
// addresses locally instead of the persistent loops hoisting them (and spilling them) for the
// whole instance.
__device__ __forceinline__ int opaque_lane() {
  int l = threadIdx.x & 63;
  asm volatile("" : "+v"(l));
  return l;
}

// Order LDS traffic between lanes of the wave: DS instructions of one wave execute in order,
// so only the compiler must not move memory operations across this point.
#define WSYNC() asm volatile("" ::: "memory")

// ------------------------------------------------------------------------------------------
// diagnostic build only (-DCMPC_STAMPS): per-phase s_memtime cycle totals.  Phases: 0 condense
// (+tile load), 1 invert, 2 gradient, 3 symv, 4 polish (all of it), 5 instance total,
// 6 setup, 7 ADMM iteration outside gradient/symv, 14 polish setup, 15 output (+final gradient),
// 28 face downdates (their symvs included); counters: 8 condense+invert calls, 9 polish
// attempts, 10 instances, 11 ADMM iterations, 12 gradient calls, 13 symv calls, 29 downdated
// repairs, 30 downdated faces (16-27: team-mode phases, cmpc_team.hip).
// ------------------------------------------------------------------------------------------
// every other diagnostic build (trace, counts, gres, times, poison): the Diag hooks and the
// trace macros of cmpc_diag.h
#include "cmpc_diag.h"
#ifdef CMPC_STAMPS
__device__ unsigned long long g_stamps[32];
// (fenced: outstanding memory and LDS traffic completes, no code moves across a stamp; totals
// accumulate per wave in LDS, so no contended atomic sits between two stamps)
#define CMPC_FENCE()                                            \
  do {                                                          \
    __builtin_amdgcn_sched_barrier(0);                          \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); \
    __builtin_amdgcn_sched_barrier(0);                          \
  } while (0)
#define CMPC_T0(name) \
  CMPC_FENCE();       \
  const unsigned long long name = __builtin_amdgcn_s_memtime()
#define CMPC_ACC(ph, t0)                                                              \
  do {                                                                                \
    CMPC_FENCE();                                                                     \
    const unsigned long long _t1 = __builtin_amdgcn_s_memtime();                      \
    if (threadIdx.x == 0) s.st[ph] += _t1 - (t0);                                     \
  } while (0)
#define CMPC_CNT(ph, v) \
  do { if (threadIdx.x == 0) s.st[ph] += (unsigned long long)(v); } while (0)
#else
#define CMPC_T0(name) (void)0
#define CMPC_ACC(ph, t0) (void)0
#define CMPC_CNT(ph, v) (void)0
#endif

}  // namespace cmpc
