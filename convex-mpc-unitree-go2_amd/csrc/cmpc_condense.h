// cmpc_condense.h -- the three condensations of the horizon into the register tiles.
#pragma once
#include "cmpc_instance.h"

namespace cmpc {

// ------------------------------------------------------------------------------------------
// condensation straight into the register tiles (MFMA)
// ------------------------------------------------------------------------------------------
// H = sum_t G_t' Q2 G_t + diag(Rt) + shift, where G_t (12 x n) column p is A^{t - k_p} b_p
// for k_p <= t and 0 otherwise (the prediction-matrix row block of step t).  G_t lives in
// REGISTERS as one accumulator tile per 16-column chunk (lane (g, c): states 4g..4g+3 of
// column 16 J + c), with the state index permuted k = 4g + q across the four MFMA steps so that
// an accumulator is directly the next product's B operand: G_{t+1} = A G_t is a chain of four
// MFMAs per chunk, and every lower tile (I, J) accumulates (Q2 G_t)_I' (G_t)_J with four MFMAs
// whose accumulator IS the matrix tile.  Tile row I starts to receive terms at the step of its
// first parameter; nothing of G ever goes through memory.
// + diag(Rt) + shift, identity on padding.  Only the diagonal tiles and the tile rows that reach
// the padding (a lower tile's padded columns imply padded rows) have anything to change: the
// interior off-diagonal tiles are skipped by a uniform test instead of testing every element.
// The elements that remain are settled by selects, not branches.  A lane holds a diagonal element
// only where c >> 2 == g, and then it is that of row 16 I + c: one read of Rt per tile row (its
// value is unused in the other lanes; four rows per lane as one 16-byte read cost the NC 128
// kernel five more spilled registers).  A diagonal element takes v + (Rt + shift), padding takes
// the identity, and every other element keeps its value (selected, not v + 0: a -0 stays -0).
// Per element branches cost a trot instance 32 serial LDS round trips and ~300 exec branches here.
template <int NC>
__device__ __forceinline__ void condense_finish(Smem<NC>& s, f4 (&M)[Cfg<NC>::NTL], int n,
                                                float shift) {
  using C = Cfg<NC>;
  const int lane = opaque_lane();
  const int g = lane >> 4, c = lane & 15;
#pragma unroll
  for (int I = 0; I < C::TT; ++I) {
    const float rs = s.Rt[16 * I + c] + shift;
#pragma unroll
    for (int J = 0; J <= I; ++J) {
      if (J != I && 16 * I + 16 <= n) continue;  // uniform: interior off-diagonal tile
      f4 v = M[tile_index(I, J)];
      const int col = 16 * J + c;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = 16 * I + 4 * g + q;
        const bool pad = row >= n || col >= n;
        if (J == I) {  // compile-time after unrolling
          const bool dg = 4 * g + q == c;
          const float dv = v[q] + rs;
          v[q] = pad ? (dg ? 1.f : 0.f) : (dg ? dv : v[q]);
        } else {
          v[q] = pad ? 0.f : v[q];
        }
      }
      M[tile_index(I, J)] = v;
    }
  }
  WSYNC();
}

// ---- building blocks of the condensations, shared by the one-wave forms below and the team's
// per-slot form (cmpc_team.hip team_factor) ----
// K = 12 state layout of every product over the states: position (g, q) of a 16-row chunk holds
// state 3g + q for q < 3, and q = 3 is padding in every lane group, so the fourth K = 4 slice of
// each product is all zeros and is skipped: three MFMAs per product instead of four.  The state
// of output row / lane column c (-1: padding):
__device__ __forceinline__ int lane_state(int c) {
  return ((c & 3) < 3) ? 3 * (c >> 2) + (c & 3) : -1;
}
// aA = A[sc][3g + q] (A operand of A X), aT = A[3g + q][sc] (of A' X), q2 = Q2 as an
// accumulator tile (diagonal)
template <class SM>
__device__ __forceinline__ void state_operands(SM& s, int g, int c, float (&aA)[3],
                                               float (&aT)[3], f4& q2) {
  const int sc = lane_state(c);
  q2 = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int r = 3 * g + q;
    aA[q] = (sc >= 0) ? s.A[sc * 12 + r] : 0.f;
    aT[q] = (sc >= 0) ? s.A[r * 12 + sc] : 0.f;
    q2[q] = (r == sc) ? s.Q2[r] : 0.f;
  }
}

// Block-row form, backward pass.  C_i = P_i B_i on column chunk J (P symmetric, so its
// accumulator layout is also its A-operand layout), stored param-major [p][12] for step i's own
// params p0 .. p1 - 1
template <class SM>
__device__ __forceinline__ void blockrow_C_chunk(SM& s, float* Cs, const f4& Pt, int J, int p0,
                                                 int p1, int n, int g, int c) {
  const int p = 16 * J + c;
  float bt[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) bt[q] = s.Bt[p * kBS + 3 * g + q];
  f4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 3; ++q) d = mfma4(Pt[q], (p < n) ? bt[q] : 0.f, d);
  if (p >= p0 && p < p1) {
#pragma unroll
    for (int q = 0; q < 3; ++q) Cs[p * 12 + 3 * g + q] = d[q];
  }
}
// P <- Q2 + A' P A
__device__ __forceinline__ void blockrow_P_step(f4& Pt, const float (&aT)[3], const f4& q2) {
  f4 y = {0.f, 0.f, 0.f, 0.f}, z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 3; ++q) y = mfma4(Pt[q], aT[q], y);  // Y = P A
#pragma unroll
  for (int q = 0; q < 3; ++q) z = mfma4(aT[q], y[q], z);   // Z = A' Y
#pragma unroll
  for (int q = 0; q < 4; ++q) Pt[q] = z[q] + q2[q];
}

template <int NC>
__device__ __forceinline__ void condense_tiles_fwd(Smem<NC>& s, const KParams& P,
                                                   f4 (&M)[Cfg<NC>::NTL], int n, float shift) {
  using C = Cfg<NC>;
  const int lane = opaque_lane();
  const int g = lane >> 4, c = lane & 15;
  const int N = P.N;
  n = uniform(n);
#pragma unroll
  for (int t = 0; t < C::NTL; ++t) M[t] = f4{0.f, 0.f, 0.f, 0.f};
  // (Q2 scales the A operand here, as Q2[3g + q], so state_operands' tile form does not apply)
  float aA[3], q2[3];  // A operand of A G: A[sc][3g + q]; Q2[3g + q]
  const int sc = lane_state(c);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int r = 3 * g + q;
    aA[q] = (sc >= 0) ? s.A[sc * 12 + r] : 0.f;
    q2[q] = s.Q2[r];
  }
  int kI[C::TT];  // first step of tile row I (N: no parameters)
#pragma unroll
  for (int I = 0; I < C::TT; ++I) kI[I] = (16 * I < n) ? s.par[16 * I] : N;
  f4 Gd[C::TT];
#pragma unroll
  for (int J = 0; J < C::TT; ++J) Gd[J] = f4{0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < N; ++t) {
    if (t > 0) {  // G_t = A G_{t-1} on the chunks that already hold columns
#pragma unroll
      for (int J = 0; J < C::TT; ++J) {
        if (kI[J] >= t) continue;  // uniform
        f4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 3; ++q) d = mfma4(aA[q], Gd[J][q], d);
        Gd[J] = d;
      }
    }
    // new columns b_p of step t (params off[t] .. off[t+1]-1; at most two chunks)
    const int p0 = s.off[t], p1 = s.off[t + 1];
#pragma unroll
    for (int J = 0; J < C::TT; ++J) {
      if (16 * J + 15 < p0 || 16 * J >= p1) continue;  // uniform
      const int p = 16 * J + c;
      if (p >= p0 && p < p1) {
        const float* bp = &s.Bt[p * kBS + 3 * g];
        Gd[J] = f4{bp[0], bp[1], bp[2], 0.f};
      }
    }
#pragma unroll
    for (int I = 0; I < C::TT; ++I) {
      if (kI[I] > t) continue;  // uniform: row block I has no column yet
      float a[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) a[q] = q2[q] * Gd[I][q];
#pragma unroll
      for (int J = 0; J <= I; ++J) {
        f4 acc = M[tile_index(I, J)];
#pragma unroll
        for (int q = 0; q < 3; ++q) acc = mfma4(a[q], Gd[J][q], acc);
        M[tile_index(I, J)] = acc;
      }
    }
  }
  condense_finish<NC>(s, M, n, shift);
}

// Diagonal tiles of the block-row and closed-form condensations, which fill only the entries
// whose column step <= row step: entry (r, c) with step(c) > step(r) is the mirror of (c, r).
// The tiles turn through 16 x 16 scratches in the G slab (C and V are dead by then: the tile
// loops have read them), as many at a time as the slab holds -- one write / read round trip per
// batch instead of one per tile.  A lane's four transposed entries and its four row steps are
// one 16-byte read each.
template <int NC>
__device__ __forceinline__ void mirror_diagonals(Smem<NC>& s, f4 (&M)[Cfg<NC>::NTL], int n, int N) {
  using C = Cfg<NC>;
  // tiles per batch: the fewest batches the slab allows, of equal size (NC 128: two of four)
  constexpr int kFit = 12 * NC / 256, kBatches = (C::TT + kFit - 1) / kFit;
  constexpr int BT = (C::TT + kBatches - 1) / kBatches;
  static_assert(BT >= 1 && BT * 256 <= 12 * NC, "the batch fits the G slab");
  typedef int i4 __attribute__((ext_vector_type(4)));
  const int lane = opaque_lane();
  const int g = lane >> 4, c = lane & 15;
  WSYNC();
  float* T = s.G;
#pragma unroll
  for (int I0 = 0; I0 < C::TT; I0 += BT) {
    if (16 * I0 >= n) continue;  // uniform
#pragma unroll
    for (int I = I0; I < I0 + BT && I < C::TT; ++I) {
      if (16 * I >= n) continue;  // uniform
      const f4 v = M[tile_index(I, I)];
#pragma unroll
      for (int q = 0; q < 4; ++q) T[256 * (I - I0) + (4 * g + q) * 16 + c] = v[q];
    }
    WSYNC();
#pragma unroll
    for (int I = I0; I < I0 + BT && I < C::TT; ++I) {
      if (16 * I >= n) continue;  // uniform
      f4 v = M[tile_index(I, I)];
      const int pc = 16 * I + c;
      const int kp = s.par[pc];  // (pc < NC: read whatever n is, then selected -- no exec region)
      const int kc = (pc < n) ? kp : N;
      const i4 kr4 = *reinterpret_cast<const i4*>(&s.par[16 * I + 4 * g]);
      const f4 tr = *reinterpret_cast<const f4*>(&T[256 * (I - I0) + c * 16 + 4 * g]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int pr = 16 * I + 4 * g + q;
        const int kr = (pr < n) ? kr4[q] : N;
        v[q] = (kc > kr) ? tr[q] : v[q];
      }
      M[tile_index(I, I)] = v;
    }
    WSYNC();
  }
}

// Block-row condensation: the lower blocks of the same H are
//   H[rows of step i, cols of step j <= i] = C_i' A^{i-j} B_j,   C_i = P_i B_i,
//   P_i = sum_{t >= i} (A^{t-i})' Q2 A^{t-i} = Q2 + A' P_{i+1} A,
// so step i only adds its own 1-2 tile rows (C_i' G_i, G_i = [A^{i-j} B_j]_{j <= i} as above)
// instead of every active tile: ~25 % fewer MFMAs at n = 120.  A backward pass builds P_i in one
// accumulator tile (A' P A: eight MFMAs; P is symmetric, so its accumulator layout is also its
// A-operand layout) and stores C_i, param-major, in the G slab.  Diagonal tiles then receive
// only the entries whose column step <= row step; the others are mirrored across.
template <int NC>
__device__ __forceinline__ void condense_tiles_bc(Smem<NC>& s, const KParams& P,
                                                  f4 (&M)[Cfg<NC>::NTL], int n, float shift) {
  using C = Cfg<NC>;
  const int lane = opaque_lane();
  const int g = lane >> 4, c = lane & 15;
  const int N = P.N;
  n = uniform(n);
#pragma unroll
  for (int t = 0; t < C::NTL; ++t) M[t] = f4{0.f, 0.f, 0.f, 0.f};
  float aA[3], aT[3];
  f4 q2;
  state_operands(s, g, c, aA, aT, q2);
  float* Cs = s.G;  // C_i columns, param-major [p][12] (the G slab is free while condensing)
  // ---- backward: P_i and C_i = P_i B_i for i = N-1 .. 0 ----
  f4 Pt = q2;  // P_{N-1} = Q2 (diagonal)
  WSYNC();
  for (int i = N - 1; i >= 0; --i) {
    const int p0 = s.off[i], p1 = s.off[i + 1];
#pragma unroll
    for (int J = 0; J < C::TT; ++J) {
      if (16 * J + 15 < p0 || 16 * J >= p1) continue;  // uniform: chunks holding step i's params
      blockrow_C_chunk(s, Cs, Pt, J, p0, p1, n, g, c);
    }
    if (i > 0) blockrow_P_step(Pt, aT, q2);
  }
  WSYNC();
  // ---- forward: G_t = A G_{t-1} + new columns; rows of step t += C_t' G_t ----
  int kI[C::TT];
#pragma unroll
  for (int I = 0; I < C::TT; ++I) kI[I] = (16 * I < n) ? s.par[16 * I] : N;
  f4 Gd[C::TT];
#pragma unroll
  for (int J = 0; J < C::TT; ++J) Gd[J] = f4{0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < N; ++t) {
    if (t > 0) {
#pragma unroll
      for (int J = 0; J < C::TT; ++J) {
        if (kI[J] >= t) continue;  // uniform
        f4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 3; ++q) d = mfma4(aA[q], Gd[J][q], d);
        Gd[J] = d;
      }
    }
    const int p0 = s.off[t], p1 = s.off[t + 1];
#pragma unroll
    for (int J = 0; J < C::TT; ++J) {
      if (16 * J + 15 < p0 || 16 * J >= p1) continue;  // uniform
      const int p = 16 * J + c;
      if (p >= p0 && p < p1) {
        const float* bp = &s.Bt[p * kBS + 3 * g];
        Gd[J] = f4{bp[0], bp[1], bp[2], 0.f};
      }
    }
#pragma unroll
    for (int I = 0; I < C::TT; ++I) {
      if (16 * I + 15 < p0 || 16 * I >= p1) continue;  // uniform: tile rows holding step t
      const int p = 16 * I + c;
      float a[3] = {0.f, 0.f, 0.f};
      if (p >= p0 && p < p1) {
#pragma unroll
        for (int q = 0; q < 3; ++q) a[q] = Cs[p * 12 + 3 * g + q];
      }
#pragma unroll
      for (int J = 0; J <= I; ++J) {
        f4 acc = M[tile_index(I, J)];
#pragma unroll
        for (int q = 0; q < 3; ++q) acc = mfma4(a[q], Gd[J][q], acc);
        M[tile_index(I, J)] = acc;
      }
    }
  }
  mirror_diagonals<NC>(s, M, n, N);
  condense_finish<NC>(s, M, n, shift);
}

// Closed-form condensation for a nilpotent step matrix (round 4).  The reference discretises a
// nilpotent Ac (Ac^2 = 0: its only blocks map velocity to position and omega to the Euler
// rates), so its zero-order hold is exactly A = I + N with N = Ac dt and N^2 = 0
// (com_trajectory.py:272-286; cmpc_build_dynamics).  Then A^j = I + j N and the
// prediction column of param p (step k_p) at step t >= k_p is affine in t:
//     A^{t - k_p} b_p = U_p + t V_p,   V_p = N b_p,   U_p = b_p - k_p V_p,
// so  H[p][p'] = sum_{t >= m} (U_p + t V_p)' Q2 (U_p' + t V_p'),  m = max(k_p, k_p'),
//              = X_p' U_p' + Y_p' V_p'   with   X_p = Q2 (S0 U_p + S1 V_p),
//                                               Y_p = Q2 (S1 U_p + S2 V_p),
// S_i = sum_{t=m}^{N-1} t^i, whenever m = k_p (the row param's step).  Params are ordered by
// step, so that holds for every entry of an off-diagonal tile (rows later than columns) and for
// the lower part of a diagonal tile; the rest of a diagonal tile is mirrored, as in the
// block-row form.  Every tile is then SIX MFMAs (two K = 12 products, 3 each) instead of the
// three per active step of the forward form: ~240 MFMAs for n = 120 instead of 1,248 (936 in
// the block-row form), with V = N b three MFMAs per 16-param chunk, kept in registers.  fp32
// error on the fixture matrices (unit-diagonal scaled, vs float64): 2.6e-7 against 4.1e-7 for
// the step-by-step products.  The solve checks N^2 = 0 exactly per instance (nilpotent_step);
// any other A takes the general forms above.
// Sums over the horizon's remaining steps t = k .. N-1 of 1, t and t^2 (condense_tiles_nil), as
// exact integers
__device__ __forceinline__ void step_sums(int k, int N, float& S0, float& S1, float& S2) {
  S0 = (float)(N - k);
  S1 = (float)((N * (N - 1) - k * (k - 1)) >> 1);
  S2 = (float)(((N - 1) * N * (2 * N - 1) - (k - 1) * k * (2 * k - 1)) / 6);
}

template <int NC>
__device__ __forceinline__ void condense_tiles_nil(Smem<NC>& s, const KParams& P,
                                                   f4 (&M)[Cfg<NC>::NTL], int n, float shift) {
  using C = Cfg<NC>;
  const int lane = opaque_lane();
  const int g = lane >> 4, c = lane & 15;
  const int N = P.N;
  n = uniform(n);
  const int TA = (n + 15) >> 4;
  float q2[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) q2[q] = s.Q2[3 * g + q];
  // The column operands (u, v) of every chunk, once: each is reused by every tile row below it
  // (loaded per tile instead: 7 LDS reads between every tile's MFMAs; caching them took config 3
  // 9.09 -> 8.60 ms, config 2 at 65,536 10.55 -> 9.99 ms, A/B in one GPU visit), and the
  // chunk's step k: the tile row I = J below takes its sums over the steps from it, not from
  // another LDS read per tile row.
  // V = N b is three MFMAs per chunk, and lane (g, c) receives exactly the entries of V it uses as
  // its own column operand (states 3g .. 3g + 2 of param 16 J + c): V stays in registers and never
  // goes through the G slab.  The chunk's Bt column and step are read once, for V and for u, at
  // p < NC whatever n is, and what lies past n is settled by selects: a read under `p < n` is an
  // exec region of its own with its own wait, which was four serial LDS round trips per chunk.
  float uc[C::TT][3], vc[C::TT][3];
  int kc[C::TT];
  {
    // K = 12 state layout (as condense_tiles_fwd): accumulator position 4g + q holds state 3g + q
    const int sc = lane_state(c);
    float aN[3];  // A operand of N X: N[sc][3g + q]
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int r = 3 * g + q;
      aN[q] = (sc >= 0) ? s.A[sc * 12 + r] - ((sc == r) ? 1.f : 0.f) : 0.f;
    }
    WSYNC();
#pragma unroll
    for (int J = 0; J < C::TT; ++J) {
      if (J >= TA) {  // uniform: a padding chunk
        kc[J] = 0;
#pragma unroll
        for (int q = 0; q < 3; ++q) vc[J][q] = uc[J][q] = 0.f;
        continue;
      }
      const int p = 16 * J + c;
      const bool ok = p < n;
      const int kp = s.par[p];
      float bp[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) bp[q] = s.Bt[p * kBS + 3 * g + q];
      kc[J] = ok ? kp : 0;
      const float kf = (float)kc[J];
      f4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 3; ++q) d = mfma4(aN[q], ok ? bp[q] : 0.f, d);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        vc[J][q] = ok ? d[q] : 0.f;
        uc[J][q] = ok ? fmaf(-kf, vc[J][q], bp[q]) : 0.f;
      }
    }
  }
#pragma unroll
  for (int I = 0; I < C::TT; ++I) {
    if (I >= TA) {  // uniform: a padding tile row receives no product
#pragma unroll
      for (int J = 0; J <= I; ++J) M[tile_index(I, J)] = f4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    float x[3], y[3];
    {
      float S0, S1, S2;  // sum_{t=k}^{N-1} 1, t, t^2
      step_sums(kc[I], N, S0, S1, S2);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        // the row's (u, v) are its chunk's column operands: the same expression on the same
        // values, so they are taken from uc / vc instead of seven more LDS reads per tile row
        const float v = vc[I][q];
        const float u = uc[I][q];
        x[q] = q2[q] * fmaf(S0, u, S1 * v);
        y[q] = q2[q] * fmaf(S1, u, S2 * v);
      }
    }
#pragma unroll
    for (int J = 0; J <= I; ++J) {
      float u[3], v[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        u[q] = uc[J][q];
        v[q] = vc[J][q];
      }
      // the tile's first product starts from a zero accumulator operand (0 + x u rounds as the
      // accumulate into a zeroed tile did): no tile is zeroed before the loop
      f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 3; ++q) acc = mfma4(x[q], u[q], acc);
#pragma unroll
      for (int q = 0; q < 3; ++q) acc = mfma4(y[q], v[q], acc);
      M[tile_index(I, J)] = acc;
    }
  }
  mirror_diagonals<NC>(s, M, n, N);
  condense_finish<NC>(s, M, n, shift);
}

// Is the step matrix A = I + N with N^2 = 0 exactly (the reference's discretisation)?  Then
// condense_tiles_nil applies.  Uniform.
template <class SM>
__device__ __forceinline__ bool nilpotent_step(SM& s) {
  const int lane = opaque_lane();
  WSYNC();
  // Lane 4 i + c (i < 12, c < 3) takes the elements (i, 4 c .. 4 c + 3) of N^2: row i of A once
  // and the four entries of every row k, all as 16-byte reads (15 per lane, one trip; an element
  // per lane took 24 four-byte reads in each of three trips).  Every element is the same
  // products summed over k ascending.
  const int i = lane >> 2, c = lane & 3;
  bool nz = false;
  if (lane < 48 && c < 3) {
    f4 ni[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      ni[q] = *reinterpret_cast<const f4*>(&s.A[12 * i + 4 * q]);
#pragma unroll
      for (int j = 0; j < 4; ++j) ni[q][j] -= (i == 4 * q + j) ? 1.f : 0.f;
    }
    f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const f4 nk = *reinterpret_cast<const f4*>(&s.A[12 * k + 4 * c]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = fmaf(ni[k >> 2][k & 3], nk[j] - ((k == 4 * c + j) ? 1.f : 0.f), acc[j]);
    }
    nz = acc[0] != 0.f || acc[1] != 0.f || acc[2] != 0.f || acc[3] != 0.f;
  }
  return __any(nz) == 0;
}

// Which condensation: the closed form for a nilpotent step (nil); otherwise the block-row form
// has ~25 % fewer MFMAs but longer dependency chains.  With one wave per SIMD (small batches,
// latency) the chains are what a wave waits on either way and the fewer MFMAs win (B = 256:
// 0.61 -> 0.48 ms); with two busy waves per SIMD the forward form keeps the matrix pipe ~80 %
// busy and is ~5 % faster.
template <int NC>
__device__ __forceinline__ void condense_tiles(Smem<NC>& s, const KParams& P,
                                               f4 (&M)[Cfg<NC>::NTL], int n, float shift,
                                               bool nil = false) {
  if (nil) {  // uniform
    condense_tiles_nil<NC>(s, P, M, n, shift);
    return;
  }
  if constexpr (NC <= 128) {  // the 1-wave-per-SIMD bins would spill the second form
    if (P.latency_mode) {  // uniform
      condense_tiles_bc<NC>(s, P, M, n, shift);
      return;
    }
  }
  condense_tiles_fwd<NC>(s, P, M, n, shift);
}

}  // namespace cmpc
