// cmpc_factor.h -- block LDL' by the sweep operator, its solve, and the park slab moves.
#pragma once
#include "cmpc_instance.h"

namespace cmpc {

// Element c & 3 of a diagonal tile's register: the matrix diagonal in the lanes with c >> 2 == g
// (lane (g, c) holds rows 4g .. 4g + 3 of column c), by selects
__device__ __forceinline__ float diag_element(const f4& d, int c) {
  const int qs = c & 3;
  return qs == 0 ? d[0] : qs == 1 ? d[1] : qs == 2 ? d[2] : d[3];
}

// ---- software-pipelined sweep (bins up to kSweepPipeMaxNC; measured +3-5 % on NC = 128, and
// -5 % on cfg2 when also used for the 1-wave-per-SIMD bins, whose registers it spills) ----
constexpr int kSweepPipeMaxNC = 128;
// The next 4-pivot step reads only the tiles of its pivot row/column block ("critical" tiles).
// Each step issues its MFMAs on those tiles first, publishes the next panel from them, and then
// issues the remaining MFMAs of the step in the same basic block as the next step's LDL and
// operand build, so that serial chain fills the gaps between MFMAs instead of stalling the wave.
template <int NC, int K, class SM>
__device__ __forceinline__ void sweep_publish(SM& s, const f4 (&M)[Cfg<NC>::NTL], int sub,
                                              int g, int c) {
  using C = Cfg<NC>;
  const int c0 = 4 * sub;
  const int pc = c - c0;
  const bool colw = pc >= 0 && pc < 4;
  if (colw) {
#pragma unroll
    for (int I = K; I < C::TT; ++I) {
      f4 m = M[tile_index(I, K)];
      if (I == K) {
#pragma unroll
        for (int q = 0; q < 4; ++q) m[q] -= (4 * g + q == c) ? 1.f : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) s.pan[(16 * I + 4 * g + q) * 4 + pc] = m[q];
    }
  }
  // (the factorization never reads the swept rows above the block)
  WSYNC();
}

// LDL' of the 4x4 pivot block Dm (row-major): D = L diag(dl) L' with unit lower L, factored
// redundantly in every lane, so P^ D^-1 P^' = Y diag(1/dl) Y' with Y = P^ L^-T: the columns of Y
// are the pivot columns as the scalar sweep would see them (each already eliminated by the earlier
// pivots of the step), which keeps the scalar sweep's accuracy.  Lane group g takes its row of
// L^-1 (w0..w3) and ig = 1/dl_g, selected once per step, so each panel row costs four FMAs and no
// branches (panel_row).  (Results through references: returned as a struct, the compiler spilled
// an operand in every sweep step, 28 scratch stores and loads in the NC <= 128 kernel.)
__device__ __forceinline__ void pivot_block(const float (&Dm)[16], int g, float& w0, float& w1,
                                            float& w2, float& w3, float& ig) {
  const bool g1 = g == 1, g2 = g == 2, g3 = g == 3;
  const float i0 = __builtin_amdgcn_rcpf(Dm[0]);
  const float l10 = Dm[4] * i0, l20 = Dm[8] * i0, l30 = Dm[12] * i0;
  const float i1 = __builtin_amdgcn_rcpf(Dm[5] - l10 * Dm[4]);
  const float u21 = Dm[9] - l20 * Dm[4], u31 = Dm[13] - l30 * Dm[4];
  const float l21 = u21 * i1, l31 = u31 * i1;
  const float i2 = __builtin_amdgcn_rcpf(Dm[10] - l20 * Dm[8] - l21 * u21);
  const float u32 = Dm[14] - l30 * Dm[8] - l31 * u21;
  const float l32 = u32 * i2;
  const float i3 = __builtin_amdgcn_rcpf(Dm[15] - l30 * Dm[12] - l31 * u31 - l32 * u32);
  const float n10 = -l10, n21 = -l21, n32 = -l32;
  const float n20 = l21 * l10 - l20, n31 = l32 * l21 - l31;
  const float n30 = -l30 - l31 * n10 - l32 * n20;
  w0 = g3 ? n30 : g2 ? n20 : g1 ? n10 : 1.f;
  w1 = g3 ? n31 : g2 ? n21 : g1 ? 1.f : 0.f;
  w2 = g3 ? n32 : g2 ? 1.f : 0.f;
  w3 = g3 ? 1.f : 0.f;
  ig = g3 ? i3 : g2 ? i2 : g1 ? i1 : i0;
}
// y_g = (P^ L^-T)_g = sum_m L^-1[g][m] P^_m of one panel row ph
__device__ __forceinline__ float panel_row(const f4& ph, float w0, float w1, float w2, float w3) {
  return fmaf(w3, ph[3], fmaf(w2, ph[2], fmaf(w1, ph[1], w0 * ph[0])));
}

// The pivot block (rows k0..k0+3 of the panel) and the step's MFMA operands: A = -Y rows,
// B = diag(1/dl) Y' columns
template <int NC, int KMIN, class SM>
__device__ __forceinline__ void sweep_operands(SM& s, int k0, int g, int c,
                                               float (&a)[Cfg<NC>::TT], float (&b)[Cfg<NC>::TT]) {
  using C = Cfg<NC>;
  float Dm[16];  // the panel holds P^ = P - I: add the identity back for D
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f4 rrow = *reinterpret_cast<const f4*>(&s.pan[(k0 + i) * 4]);
#pragma unroll
    for (int j = 0; j < 4; ++j) Dm[i * 4 + j] = (i == j) ? rrow[j] + 1.f : rrow[j];
  }
  f4 ph[C::TT];
#pragma unroll
  for (int I = KMIN; I < C::TT; ++I) ph[I] = *reinterpret_cast<const f4*>(&s.pan[(16 * I + c) * 4]);
  float w0, w1, w2, w3, ig;
  pivot_block(Dm, g, w0, w1, w2, w3, ig);
#pragma unroll
  for (int I = KMIN; I < C::TT; ++I) {
    const float yg = panel_row(ph[I], w0, w1, w2, w3);
    a[I] = -yg;
    b[I] = yg * ig;
  }
}

// rank-4 update of the tiles whose criticality for pivot block Kc is CRIT
template <int NC, int Kc, bool CRIT, int KMIN>
__device__ __forceinline__ void sweep_mfma(f4 (&M)[Cfg<NC>::NTL], const float (&a)[Cfg<NC>::TT],
                                           const float (&b)[Cfg<NC>::TT], int TA) {
  using C = Cfg<NC>;
#pragma unroll
  for (int I = KMIN; I < C::TT; ++I) {
    if (I >= TA) continue;  // uniform
#pragma unroll
    for (int J = KMIN; J <= I; ++J) {
      const bool crit = J == Kc && I >= Kc;
      if (crit != CRIT) continue;  // compile-time after unrolling
      const int t = tile_index(I, J);
      M[t] = mfma4(a[I], b[J], M[t]);
    }
  }
}

template <int NC, int K>
__device__ __forceinline__ void sweep_diagfix(f4 (&M)[Cfg<NC>::NTL], int sub, int g, int c) {
  const int pc = c - 4 * sub;
  const bool roww = g == sub;
  f4& m = M[tile_index(K, K)];
#pragma unroll
  for (int q = 0; q < 4; ++q) m[q] -= (roww && pc == q) ? 2.f : 0.f;
}

template <int NC, int K, class SM>
__device__ __forceinline__ void sweep_block(SM& s, f4 (&M)[Cfg<NC>::NTL], int ng, int TA,
                                            int g, int c, float (&a)[Cfg<NC>::TT],
                                            float (&b)[Cfg<NC>::TT]) {
  using C = Cfg<NC>;
  constexpr int KM = K;  // first tile column the block's steps update
  if constexpr (K < C::TT) {
    if (4 * K < ng) {  // uniform
      const int subs = (ng - 4 * K) < 4 ? (ng - 4 * K) : 4;
      for (int sub = 0; sub < subs - 1; ++sub) {  // next step in the same pivot block
        sweep_mfma<NC, K, true, KM>(M, a, b, TA);
        sweep_diagfix<NC, K>(M, sub, g, c);
        sweep_publish<NC, K>(s, M, sub + 1, g, c);
        sweep_mfma<NC, K, false, KM>(M, a, b, TA);
        sweep_operands<NC, KM>(s, 16 * K + 4 * (sub + 1), g, c, a, b);
      }
      {  // last step of the block: the next step opens block K + 1
        const int sub = subs - 1;
        const bool has_next = 4 * (K + 1) < ng;
        sweep_mfma<NC, K + 1, true, KM>(M, a, b, TA);
        if constexpr (K + 1 < C::TT) {
          if (has_next) sweep_publish<NC, K + 1>(s, M, 0, g, c);
        }
        sweep_mfma<NC, K + 1, false, KM>(M, a, b, TA);
        sweep_diagfix<NC, K>(M, sub, g, c);
        if constexpr (K + 1 < C::TT) {
          if (has_next) sweep_operands<NC, K + 1>(s, 16 * (K + 1), g, c, a, b);
        }
      }
    }
    sweep_block<NC, K + 1>(s, M, ng, TA, g, c, a, b);
  }
}

// The plain sweep of the bins above kSweepPipeMaxNC: each 4-pivot step publishes its panel,
// builds its operands, updates every tile right of the swept pivots and fixes the pivot diagonals.
// The pivot-block column K is a template constant, so the panel publish, the P^ identity and the
// diagonal fix address their tiles directly (no runtime dispatch over register tiles); the four
// 4-pivot steps inside a tile column are a runtime loop.
template <int NC, int K, class SM>
__device__ __forceinline__ void sweep_block_plain(SM& s, f4 (&M)[Cfg<NC>::NTL], int ng, int TA,
                                                  int g, int c) {
  using C = Cfg<NC>;
  if constexpr (K < C::TT) {
    if (4 * K < ng) {  // uniform
      const int subs = (ng - 4 * K) < 4 ? (ng - 4 * K) : 4;
      for (int sub = 0; sub < subs; ++sub) {
        float a[C::TT], b[C::TT];
        sweep_publish<NC, K>(s, M, sub, g, c);
        sweep_operands<NC, K>(s, 16 * K + 4 * sub, g, c, a, b);
        sweep_mfma<NC, -1, false, K>(M, a, b, TA);  // Kc = -1: no tile is critical, so every tile
        sweep_diagfix<NC, K>(M, sub, g, c);
      }
    }
    sweep_block_plain<NC, K + 1>(s, M, ng, TA, g, c);
  }
}

// The scaling and un-scaling passes of ldl_tiles form m[q] *= r[q] * cj on register pairs (q = 0, 1
// and q = 2, 3): v_pk_mul_f32 rounds each half as the scalar multiply does, and the two passes are
// 8 NTL multiplies per lane otherwise.  Not in the NC 192 kernel, which the pairs' temporaries
// took from 0 to 40 spilled registers.
template <int NC>
constexpr bool kPackedScale = NC <= 160;
__device__ __forceinline__ void scale_tile(f4& m, f2 t01, f2 t23) {
  const f2 m01 = f2{m[0], m[1]} * t01, m23 = f2{m[2], m[3]} * t23;
  m = f4{m01[0], m01[1], m23[0], m23[1]};
}

// ------------------------------------------------------------------------------------------
// block LDL' factorization by the sweep operator (4 pivots per step, MFMA rank-4 updates)
// ------------------------------------------------------------------------------------------
// The symmetric sweep restricted to the tiles right of the swept pivots (round 5; rounds 1-4
// swept every tile into the explicit inverse): a block LDL' factorization with 16-pivot blocks,
// 4 T(TT - K) MFMAs per block K instead of 4 NTL (T(m) = m (m + 1) / 2: 480 instead of 1,152 for
// NC = 128).  Sweeping block K on rows / columns >= 16 K leaves -D_K^-1 in tile (K, K) (D_K the
// Schur-complemented pivot block), L_IK = H_IK D_K^-1 in the tiles below it, and the Schur
// complement to its right; unscaled, tile (K, K) holds D_K^-1 and tiles (I > J) the unit
// block-lower L of H = L D L' (applied by ldl_apply).
template <int NC, class SM>
__device__ __forceinline__ void ldl_tiles(SM& s, f4 (&M)[Cfg<NC>::NTL], int n) {
  using C = Cfg<NC>;
  const int lane = opaque_lane();
  const int g = lane >> 4, c = lane & 15;
  n = uniform(n);
  const int TA = (n + 15) >> 4;
  // unit-diagonal scaling (padding: 1): the lanes with c >> 2 == g hold the diagonal, as
  // element c & 3 -- one select, one rsqrt and one masked store per tile row
#pragma unroll
  for (int I = 0; I < C::TT; ++I) {
    const float dg = diag_element(M[tile_index(I, I)], c);
    const int p = 16 * I + c;
    const float r = (p < n && dg > 0.f) ? rsqrtf(dg) : 1.f;
    if ((c >> 2) == g) s.ds[p] = r;
  }
  WSYNC();
#pragma unroll
  for (int I = 0; I < C::TT; ++I) {
    const f4 ri = *reinterpret_cast<const f4*>(&s.ds[16 * I + 4 * g]);
#pragma unroll
    for (int J = 0; J <= I; ++J) {
      const float cj = s.ds[16 * J + c];
      f4& m = M[tile_index(I, J)];
      if constexpr (kPackedScale<NC>) {
        scale_tile(m, f2{ri[0], ri[1]} * f2{cj, cj}, f2{ri[2], ri[3]} * f2{cj, cj});
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) m[q] *= ri[q] * cj;
      }
    }
  }
  const int ng = (n + 3) >> 2;
  if constexpr (NC <= kSweepPipeMaxNC) {
    if (ng > 0) {
      float a[C::TT], b[C::TT];
      sweep_publish<NC, 0>(s, M, 0, g, c);
      sweep_operands<NC, 0>(s, 0, g, c, a, b);
      sweep_block<NC, 0>(s, M, ng, TA, g, c, a, b);
    }
  } else {
    sweep_block_plain<NC, 0>(s, M, ng, TA, g, c);
  }
  // undo the scaling: the diagonal tiles hold -(scaled D_K^-1), the tiles below them the
  // scaled L~ = S^-1 L S.  There are only NC distinct reciprocals 1 / ds[p]: each is divided out
  // once, by lane p % 64, and a lane reads its four as one 16-byte read per tile row (every lane
  // dividing its own four per tile row was 4 TT full-precision divisions per lane).  They go
  // through the panel, which is the sweep's own scratch: its last read is the last pivot step's,
  // above, and nothing outside the sweep reads it before writing it.
  float* rinvs = s.pan;
  WSYNC();
  // (the lane's coordinates re-derived: the sweep's do not stay live into this pass, which left
  // the NC 192 kernel without a spilled register)
  const int lane_r = opaque_lane();
  const int g_r = lane_r >> 4, c_r = lane_r & 15;
#pragma unroll
  for (int p0 = 0; p0 < NC; p0 += 64) {
    const int p = p0 + lane_r;
    if (p < NC) rinvs[p] = 1.f / s.ds[p];
  }
  WSYNC();
#pragma unroll
  for (int I = 0; I < C::TT; ++I) {
    const f4 ri = *reinterpret_cast<const f4*>(&s.ds[16 * I + 4 * g_r]);
    const f4 rinv = *reinterpret_cast<const f4*>(&rinvs[16 * I + 4 * g_r]);
#pragma unroll
    for (int J = 0; J <= I; ++J) {
      const float cj = s.ds[16 * J + c_r];
      f4& m = M[tile_index(I, J)];
      if constexpr (!kPackedScale<NC>) {
#pragma unroll
        for (int q = 0; q < 4; ++q) m[q] *= (J < I) ? rinv[q] * cj : -(ri[q] * cj);
      } else if (J < I) {  // compile-time after unrolling
        scale_tile(m, f2{rinv[0], rinv[1]} * f2{cj, cj}, f2{rinv[2], rinv[3]} * f2{cj, cj});
      } else {
        scale_tile(m, -(f2{ri[0], ri[1]} * f2{cj, cj}), -(f2{ri[2], ri[3]} * f2{cj, cj}));
      }
    }
  }
}

// out = (L D L')^-1 in over the first n params (factors from ldl_tiles; out is
// zero beyond n): z = L^-1 in block row by block row (row sums over the block's columns), then
// x = L'^-1 D^-1 z from the last block row up (column sums over the row's 4-lane groups); each
// block's result turns layout (rows <-> columns) through `out`, which holds z, then x.
template <int NC, class SM>
__device__ __forceinline__ void ldl_apply(SM& s, const f4 (&M)[Cfg<NC>::NTL], int n,
                                          const float* in, float* out) {
  using C = Cfg<NC>;
  CMPC_T0(t_sv);
  const int lane = opaque_lane();
  const int g = lane >> 4, c = lane & 15;
  n = uniform(n);
  const int TA = (n + 15) >> 4;
  WSYNC();
  float zc[C::TT];  // z by block, column layout (lane c: z[16 J + c])
  // backward accumulators (column layout, per lane before the 4-group sum): sum_J L_JI' x_J
  // as each x_J is known
  float bc[C::TT];
#pragma unroll
  for (int I = 0; I < C::TT; ++I) bc[I] = 0.f;
  // `out` is zeroed once (it is never `in`): the block rows past the last real one stay so, and
  // both loops leave them alone
  if (4 * lane < NC) *reinterpret_cast<f4*>(&out[4 * lane]) = f4{0.f, 0.f, 0.f, 0.f};
  // Only the last real block row has padding rows.  Its row masks, once per call: row 4 g + q of
  // block TA - 1 for the forward pass, row c for the backward one; every block row above it is
  // kept whole by the uniform test.
  const int nl = n - 16 * (TA - 1);
  const bool kr0 = 4 * g < nl, kr1 = 4 * g + 1 < nl, kr2 = 4 * g + 2 < nl, kr3 = 4 * g + 3 < nl;
  const bool kc = c < nl;
  // Forward, one block row ahead: the products of block row I + 1 with z_0 .. z_{I-1} are formed
  // in block row I's basic block (each accumulator still in J order), beside the chain z_{I-1}
  // -> z_I, which then holds only the last tile's FMAs, the row sums and the turn.  (Every block
  // row's accumulators started as soon as each z_J is known would be 4 (TT - 1) live registers.)
  f2 a01 = {0.f, 0.f}, a23 = {0.f, 0.f};  // block row I's products with z_0 .. z_{I-2}
#pragma unroll
  for (int I = 0; I < C::TT; ++I) {
    if (I >= TA) continue;  // uniform
    f4 zr = *reinterpret_cast<const f4*>(&in[16 * I + 4 * g]);
    f2 n01 = {0.f, 0.f}, n23 = {0.f, 0.f};
    if (I > 0) {
      const f4 ml = M[tile_index(I, I - 1)];
      const f2 zl = {zc[I - 1], zc[I - 1]};
      const f2 r01 = __builtin_elementwise_fma(f2{ml[0], ml[1]}, zl, a01);
      const f2 r23 = __builtin_elementwise_fma(f2{ml[2], ml[3]}, zl, a23);
      if (I + 1 < C::TT) {
#pragma unroll
        for (int J = 0; J < I; ++J) {
          const f4 m = M[tile_index(I + 1, J)];
          const f2 zj = {zc[J], zc[J]};
          n01 = __builtin_elementwise_fma(f2{m[0], m[1]}, zj, n01);
          n23 = __builtin_elementwise_fma(f2{m[2], m[3]}, zj, n23);
        }
      }
      float s0 = r01[0], s1 = r01[1], s2 = r23[0], s3 = r23[1];
      row16_sum4(s0, s1, s2, s3);
      zr[0] -= s0;
      zr[1] -= s1;
      zr[2] -= s2;
      zr[3] -= s3;
    }
    a01 = n01;
    a23 = n23;
    const bool whole = I < TA - 1;  // uniform
    zr[0] = (whole | kr0) ? zr[0] : 0.f;
    zr[1] = (whole | kr1) ? zr[1] : 0.f;
    zr[2] = (whole | kr2) ? zr[2] : 0.f;
    zr[3] = (whole | kr3) ? zr[3] : 0.f;
    // the block turns from rows to columns through `out` (a register turn -- DPP / permlane
    // swaps -- measured 1.3 % slower with this arithmetic, round 5; for the one-wave class alone
    // no gain on its kernel or on the step, profiles/heavy_paths_ab.txt)
    if (c == 0) *reinterpret_cast<f4*>(&out[16 * I + 4 * g]) = zr;
    WSYNC();
    zc[I] = out[16 * I + c];
  }
  // backward: x_I = D_I^-1 z_I - sum_{J > I} L_JI' x_J.  One LDS round trip per block row: z of
  // the block row above is read together with this one's x (x_I is stored over z_I only)
  f4 zr = {0.f, 0.f, 0.f, 0.f};
  if (TA > 0) zr = *reinterpret_cast<const f4*>(&out[16 * (TA - 1) + 4 * g]);  // uniform
#pragma unroll
  for (int I = C::TT - 1; I >= 0; --I) {
    if (I >= TA) continue;  // uniform
    const f4 d = M[tile_index(I, I)];
    const float t =
        fmaf(d[3], zr[3], fmaf(d[2], zr[2], fmaf(d[1], zr[1], fmaf(d[0], zr[0], -bc[I]))));
    float xc = col4_sum(t);
    xc = ((I < TA - 1) | kc) ? xc : 0.f;
    WSYNC();
    if (g == 0) out[16 * I + c] = xc;
    if (I == 0) break;
    WSYNC();
    const f4 xr = *reinterpret_cast<const f4*>(&out[16 * I + 4 * g]);
    zr = *reinterpret_cast<const f4*>(&out[16 * (I - 1) + 4 * g]);
#pragma unroll
    for (int J = 0; J < I; ++J) {
      const f4 m = M[tile_index(I, J)];
      bc[J] = fmaf(m[3], xr[3], fmaf(m[2], xr[2], fmaf(m[1], xr[1], fmaf(m[0], xr[0], bc[J]))));
    }
  }
  WSYNC();
  CMPC_ACC(3, t_sv);
  CMPC_CNT(13, 1);
}

// park / restore the register-resident inverse in the wave's global slab (uniform base,
// 32-bit lane offset: no per-tile 64-bit address registers)
template <int NC>
__device__ __forceinline__ void park_store(float* __restrict__ park, const f4 (&M)[Cfg<NC>::NTL]) {
  const int lane = opaque_lane();
#pragma unroll
  for (int t = 0; t < Cfg<NC>::NTL; ++t)
    *reinterpret_cast<f4*>(&park[t * 256 + lane * 4]) = M[t];
}

template <int NC>
__device__ __forceinline__ void park_load(const float* __restrict__ park, f4 (&M)[Cfg<NC>::NTL]) {
  const int lane = opaque_lane();
  asm volatile("s_waitcnt vmcnt(0)\n\tbuffer_inv sc1" ::: "memory");
#pragma unroll
  for (int t = 0; t < Cfg<NC>::NTL; ++t)
    M[t] = *reinterpret_cast<const f4*>(&park[t * 256 + lane * 4]);
}

}  // namespace cmpc
