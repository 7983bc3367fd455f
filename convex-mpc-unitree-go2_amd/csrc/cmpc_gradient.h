// cmpc_gradient.h -- the gradient by the error-coordinate rollout and adjoint (scans on the
// matrix cores).
#pragma once
#include "cmpc_condense.h"

namespace cmpc {

// Gradient of sum_k e_{k+1}'(Q2/2)e_{k+1} + v'(Rt/2)v in the current param basis
// (e by the error-coordinate rollout).  Leaves E (e_{k+1}) and L (lambda_k) in LDS.
//
// Both recursions run as log-depth scans on the matrix cores, the 12 x N state trajectory
// held as ONE accumulator tile (lane (g, c): states 4g..4g+3 of step c):
//   forward  e_{k+1} = sum_j A^{k-j} h_j :   E <- E + A^d shift_d(E),      d = 1, 2, 4, 8
//   adjoint  lambda_k = sum_j (A')^{j-k} Q2 e_{j+1} : L <- L + (A')^d shift_-d(L)
// (Hillis-Steele; the step shift is a DPP row shift, the product three MFMAs whose accumulator
// is the trajectory itself).  A^d and (A')^d come from repeated squaring in the same layout.
// powers A^d and (A')^d, d = 1, 2, 4, 8, in accumulator layout over state positions
// (pw[l][q] = A^(2^l)[state 3g+q][state of position c]); the gradient's scans use them
// (nilpotent step, s.nil: A^d = I + d N exactly, no squaring)
template <class SM>
__device__ __forceinline__ void gradient_powers(SM& s, f4 (&pw)[4], f4 (&tw)[4]) {
  const int lane = opaque_lane();
  const int g = lane >> 4, c = lane & 15;
  const int sc = lane_state(c);
  f4 Pd = {0.f, 0.f, 0.f, 0.f}, Td = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int r = 3 * g + q;
    Pd[q] = (sc >= 0) ? s.A[r * 12 + sc] : 0.f;
    Td[q] = (sc >= 0) ? s.A[sc * 12 + r] : 0.f;
  }
  pw[0] = Pd;
  tw[0] = Td;
  if (uniform(s.nil)) {
#pragma unroll
    for (int l = 1; l < 4; ++l) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float dl = (sc == 3 * g + q && q < 3) ? 1.f : 0.f;
        pw[l][q] = fmaf((float)(1 << l), Pd[q] - dl, dl);
        tw[l][q] = fmaf((float)(1 << l), Td[q] - dl, dl);
      }
    }
    return;
  }
#pragma unroll
  for (int l = 1; l < 4; ++l) {
    f4 pn = {0.f, 0.f, 0.f, 0.f}, tn = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      pn = mfma4(tw[l - 1][q], pw[l - 1][q], pn);  // A^2d  = A^d A^d   (A operand = (A^d)')
      tn = mfma4(pw[l - 1][q], tw[l - 1][q], tn);  // A'^2d = A'^d A'^d
    }
    pw[l] = pn;
    tw[l] = tn;
  }
}

// LAT (latency mode, kGradLat below): the powers come precomputed where the caller has them (team
// mode, NC <= 128: one set per instance, `pwc`/`twc`; else they are built here as in the rolled
// form), and the per-step B~ v sum is unrolled to the 12 params a step can hold so that its LDS reads
// issue together (with two busy waves per SIMD the rolled loop measured faster: issue-bound)
//
// PREC (the polish: refinement and KKT check): the rollout e_{k+1} in float64.  Its inputs are
// B_k u_k + d_k, where the legs' torques on the body (~8 rad/s per step at 200 N) cancel to a
// small e: rounded in fp32 they leave ~4e-7 of noise in the gradient, as large as the
// multiplier of a face whose release moves a force by 1e-4 relative (the direction is weighed
// only by R = 1e-5: instance 3458 of test_warm_next_tick's batch held fy at mu fz = 8 N with
// a true multiplier of -8.3e-7, optimum 7.97 N).  In float64 (products of fp32 operands are
// exact) the noise is ~5e-9; e is rounded to fp32 once and the adjoint stays fp32 (NumPy
// study: only the rollout needs the precision).  Nilpotent step only; the general A keeps the
// fp32 rollout and the relative multiplier tolerance (polish_check).
//
// Which form a kernel runs (the FMA order per lane is the same in both, so the results are
// bit-identical): the team kernels and the one-wave-per-SIMD wave kernel of NC 144 / 160
// (Cfg::WPE == 1: nothing else on the SIMD hides the rolled loop's LDS round trips; its kernel
// time -2.5 %, profiles/heavy_paths_ab.txt) take LAT.  The two-wave class keeps the rolled loop
// (issue-bound), and so does the NC 192 kernel, where LAT's 39 live operands raise the spills
// from 40 to 57 VGPRs and a standing batch gains nothing.
template <int NC, int W>
constexpr bool kGradLat = W > 1 || (Cfg<NC>::WPE == 1 && NC <= 160);
// The closing loop g = B~' lambda + R~ v with its trips unrolled (NC / 64, rounded up).  Not in
// the NC 192 kernel: its three trips' operands in flight cost 12 spilled VGPRs where it has none.
template <int NC>
constexpr bool kCloseUnrolled = NC <= 160;
// EPI (the closing loop's epilogue): called by every lane of every trip with its param p, the
// gradient entry g[p] just formed and whether p < n (else p = 0 and g[p] is meaningless); what it
// reads of param p travels with the loop's own LDS reads, and it stores only where p < n.
struct NoEpilogue {
  __device__ __forceinline__ void operator()(int, float, bool) const {}
};
template <int NC, bool LAT = false, bool PREC = false, class EPI = NoEpilogue>
__device__ __forceinline__ void gradient(Smem<NC>& s, const KParams& P, int n, const float* vin,
                                         float* gout, const f4* pwc = nullptr,
                                         const f4* twc = nullptr, EPI epi = EPI()) {
  CMPC_T0(t_gr);
  const int lane = opaque_lane();
  const int g = lane >> 4, c = lane & 15;
  const int N = P.N;
  n = uniform(n);
  WSYNC();
  // State positions (as in condense_tiles_fwd): register q of lane group g holds state 3g + q
  // (q < 3), q = 3 is padding, so every K = 16 product over states is three MFMAs (K = 12).
  // h_k = B~_k v_k + d~_k for states 3g..3g+2 of step c
  f4 Et = {0.f, 0.f, 0.f, 0.f};
  double Eh[3] = {0.0, 0.0, 0.0};  // PREC: h in float64
  if constexpr (LAT) {
    const int cc = (c < N) ? c : 0;
    const int p0 = s.off[cc], p1 = s.off[cc + 1];
    float dt[3], bv[12][3], vv[12];
#pragma unroll
    for (int q = 0; q < 3; ++q) dt[q] = s.Dt[12 * cc + 3 * g + q];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int p = min(p0 + i, NC - 1);
#pragma unroll
      for (int q = 0; q < 3; ++q) bv[i][q] = s.Bt[p * kBS + 3 * g + q];
      vv[i] = vin[p];
    }
    if constexpr (PREC) {
#pragma unroll
      for (int q = 0; q < 3; ++q) Eh[q] = (double)dt[q];
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        const bool ok = p0 + i < p1;
#pragma unroll
        for (int q = 0; q < 3; ++q) Eh[q] = ok ? fma((double)bv[i][q], (double)vv[i], Eh[q]) : Eh[q];
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if (c >= N) Eh[q] = 0.0;
        Et[q] = (float)Eh[q];
      }
    } else {
#pragma unroll
      for (int q = 0; q < 3; ++q) Et[q] = dt[q];
#pragma unroll
      for (int i = 0; i < 12; ++i) {  // (params past the step may hold anything, even NaN: select)
        const bool ok = p0 + i < p1;
#pragma unroll
        for (int q = 0; q < 3; ++q) Et[q] = ok ? fmaf(bv[i][q], vv[i], Et[q]) : Et[q];
      }
      if (c >= N) Et = f4{0.f, 0.f, 0.f, 0.f};
    }
  } else if (c < N) {
    const int p1 = s.off[c + 1];
    if constexpr (PREC) {
#pragma unroll
      for (int q = 0; q < 3; ++q) Eh[q] = (double)s.Dt[12 * c + 3 * g + q];
      for (int p = s.off[c]; p < p1; ++p) {
        const float* bt = &s.Bt[p * kBS + 3 * g];
        const double vp = (double)vin[p];
#pragma unroll
        for (int q = 0; q < 3; ++q) Eh[q] = fma((double)bt[q], vp, Eh[q]);
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) Et[q] = (float)Eh[q];
    } else {
#pragma unroll
      for (int q = 0; q < 3; ++q) Et[q] = s.Dt[12 * c + 3 * g + q];
      for (int p = s.off[c]; p < p1; ++p) {
        const float* bt = &s.Bt[p * kBS + 3 * g];
        const float vp = vin[p];
#pragma unroll
        for (int q = 0; q < 3; ++q) Et[q] = fmaf(bt[q], vp, Et[q]);
      }
    }
  }
  if (uniform(s.nil)) {
    // Nilpotent step (A = I + N, N^2 = 0, condense_tiles_nil): A^m = I + m N, so
    //   e_{k+1} = sum_{j<=k} A^{k-j} h_j = S_k + N u_k,   S_k = sum_{j<=k} h_j,
    //                                                      u_k = sum_{j<=k} (k-j) h_j = sum_{i<k} S_i,
    //   lambda_k = R_k + N' v_k,   R_k = sum_{j>=k} w_j,   v_k = sum_{i>k} R_i,   w_j = Q2 e_{j+1}:
    // four DPP prefix / suffix scans (row_shr / row_shl, zero past the row) and three MFMAs per
    // recursion instead of twelve in a dependent chain (and no powers of A); u and v are sums of
    // sums, so nothing cancels.
    const int sc = lane_state(c);
    float aN[3], aNt[3];  // A operands of N X and N' X
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int r = 3 * g + q;
      const float dl = (sc == r) ? 1.f : 0.f;
      aN[q] = (sc >= 0) ? s.A[sc * 12 + r] - dl : 0.f;
      aNt[q] = (sc >= 0) ? s.A[r * 12 + sc] - dl : 0.f;
    }
    if constexpr (PREC) {
      // the same scans in float64; N u on the f64 matrix cores, whose D layout (row = g + 4 reg)
      // puts state 3g + reg of step c in register reg of lane (g, c), as above
      double u64[3];
      row_scan2x3<false>(Eh, u64);
      const int sr = ((c >> 2) < 3) ? 3 * (c & 3) + (c >> 2) : -1;  // state of A-operand row c
      d4 acc = {Eh[0], Eh[1], Eh[2], 0.0};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int r = 3 * g + q;
        const double a = (sr >= 0) ? (double)(s.A[sr * 12 + r] - ((sr == r) ? 1.f : 0.f)) : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, u64[q], acc, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) Et[q] = (float)acc[q];
    } else {
    // S: inclusive prefix sum over the steps (lanes c of the DPP row), u: exclusive prefix sum
    // of S; the three states' scans step together
    float S[3] = {Et[0], Et[1], Et[2]}, u[3];
    row_scan2x3<false>(S, u);
#pragma unroll
    for (int q = 0; q < 3; ++q) Et[q] = S[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) Et = mfma4(aN[q], u[q], Et);
    }
    if (c < N) {
#pragma unroll
      for (int q = 0; q < 3; ++q) s.E[12 * c + 3 * g + q] = Et[q];
    }
    // R: inclusive suffix sum, v: exclusive suffix sum of R
    float Rs[3], v[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) Rs[q] = (c < N) ? s.Q2[3 * g + q] * Et[q] : 0.f;
    row_scan2x3<true>(Rs, v);
    f4 Lt = {Rs[0], Rs[1], Rs[2], 0.f};
#pragma unroll
    for (int q = 0; q < 3; ++q) Lt = mfma4(aNt[q], v[q], Lt);
    if (c < N) {
#pragma unroll
      for (int q = 0; q < 3; ++q) s.L[12 * c + 3 * g + q] = Lt[q];
    }
  } else {
  f4 pw[4], tw[4];  // d = 1, 2, 4, 8
  if (pwc != nullptr) {  // (a compile-time constant at every call site)
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      pw[l] = pwc[l];
      tw[l] = twc[l];
    }
  } else {
    gradient_powers(s, pw, tw);
  }
  // forward scan: E[:, k] += A^d E[:, k - d]  (A operand = (A^d)' = tw)
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    if ((1 << l) >= N) break;  // uniform
    f4 sh = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 3; ++q) sh[q] = row_shift_pow2<false>(Et[q], l);  // row_shr:2^l
#pragma unroll
    for (int q = 0; q < 3; ++q) Et = mfma4(tw[l][q], sh[q], Et);
  }
  if (c < N) {
#pragma unroll
    for (int q = 0; q < 3; ++q) s.E[12 * c + 3 * g + q] = Et[q];
  }
  // adjoint: L0 = Q2 e_{k+1} (zero past the horizon), L[:, k] += (A')^d L[:, k + d]
  f4 Lt = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 3; ++q) Lt[q] = (c < N) ? s.Q2[3 * g + q] * Et[q] : 0.f;
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    if ((1 << l) >= N) break;
    f4 sh = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 3; ++q) sh[q] = row_shift_pow2<true>(Lt[q], l);  // row_shl:2^l
#pragma unroll
    for (int q = 0; q < 3; ++q) Lt = mfma4(pw[l][q], sh[q], Lt);  // A operand = A^d = ((A')^d)'
  }
  if (c < N) {
#pragma unroll
    for (int q = 0; q < 3; ++q) s.L[12 * c + 3 * g + q] = Lt[q];
  }
  }  // (general A)
  WSYNC();
  // g = B~' lambda + Rt v, 64 params per trip, predicated: a lane past n reads param 0 and
  // step 0 and stores nothing
  auto close_trip = [&](int p0) {
    const bool ok = p0 + lane < n;
    const int p = ok ? p0 + lane : 0;
    const int k = ok ? s.par[p] : 0;
    const f4* l = reinterpret_cast<const f4*>(&s.L[12 * k]);
    f2 a2 = {s.Rt[p] * vin[p], 0.f};  // packed: even and odd states in the two halves
    const f4* bt = reinterpret_cast<const f4*>(&s.Bt[p * kBS]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const f4 lv = l[j], bv = bt[j];
      a2 = __builtin_elementwise_fma(f2{bv[0], bv[1]}, f2{lv[0], lv[1]}, a2);
      a2 = __builtin_elementwise_fma(f2{bv[2], bv[3]}, f2{lv[2], lv[3]}, a2);
    }
    const float gv = a2[0] + a2[1];
    if (ok) gout[p] = gv;
    epi(p, gv, ok);
  };
  if constexpr (kCloseUnrolled<NC>) {  // n <= NC: every trip's LDS reads issue together
#pragma unroll
    for (int p0 = 0; p0 < NC; p0 += 64) close_trip(p0);
  } else {
    for (int p0 = 0; p0 < n; p0 += 64) close_trip(p0);
  }
  WSYNC();
  CMPC_ACC(2, t_gr);
  CMPC_CNT(12, 1);
}

}  // namespace cmpc
