// cmpc_vjp.hip -- gradients of a loss through the optimum on the held faces of a batch of solved
// instances: given gw = dL/dw, dL/d(x0, xref, gd, Q, R, mu, fz_min, Ad, Bd) (cmpc_vjp_run,
// include/cmpc.h).
//
// The function differentiated is cmpc_gain.hip's: w*(theta) minimises the LQ problem over the
// forces f = Z p + c that stay on the held faces.  With [[H, E'], [E, 0]] [dw; dnu] = [-gw; 0]
// every gradient is a product of the primal solution (x, u, nu) with the adjoint one
// (dx, du, dnu), and the adjoint system is the same LQ problem with other linear terms:
//   state term   gw_x,k / 2 in place of -Q xref_k      s' = q'_{k+1} + gw_x,k / 2
//   force term   r = gw_u,k / 2 (the primal has none): Z'r joins the right-hand side of the
//                solve and K_k'r joins q'_k
//   d' = 0 (no gd, no c), dx_0 = 0
// So one backward recursion serves both: column 12 of the 16-wide padding carries the primal
// affine part as in gain_kernel, column 13 the adjoint's, and the elimination takes the 26
// columns [G | 14 right-hand sides].  Then one forward pass gives (x_k, u_k) and (dx_k, du_k),
// one backward costate pass gives
//   nu_k  = Ad' nu_{k+1}  - 2Q (x_{k+1} - xref_k)
//   dnu_k = Ad' dnu_{k+1} - 2Q dx_{k+1} - gw_x,k
// and the outputs are formed as the costates are produced.  The multipliers of a leg's held
// faces come in closed form from its stationarity residual r = 2R u - Bd_k' nu (adjoint:
// 2R du + gw_u - Bd_k' dnu): nu_x = -r_x on a single-sign x face, nu_z = -r_z - sx mu r_x -
// sy mu r_y on the fz row.  A leg that holds both signs of an axis is pinned at fz = 0 whatever
// mu and fz_min are and contributes to neither.
//
// One 64-lane wave per instance, fp64 on the fp32 inputs widened exactly, staged by
// cmpc_problem.h with every load of the instance issued before the first is used.  Every sum
// runs in an order the code fixes: bitwise repeatable, independent of B, of the instance's place
// in the batch and of which outputs are asked for.  Plain stores, no atomics, no workspace.
//
// This file is compiled as part of cmpc_host.hip (single translation unit).  The staging of the
// held faces, the mask and its affine set, the recursion (gain_recursion<2>) and the forward pass
// (gain_rollout<true>) are cmpc_lq.h's, as they are in cmpc_gain.hip and cmpc_refine.hip.
#include "cmpc_lq.h"

namespace cmpc {

struct VjpArgs : HeldArgs {
  const float* gw;  // [B][24N]
  double *g_x0, *g_xref, *g_gd, *g_Q, *g_R, *g_mu, *g_fz, *g_Ad, *g_Bd;  // all nullable
};

__global__ void __launch_bounds__(64) vjp_kernel(VjpArgs a, int64_t B) {
  __shared__ ProblemLds sp;
  auto& [sBd, sAd, sXr, sGX, sQ, sR, sC] = sp;
  __shared__ float sZx[64], sZy[64];                           // per (step, leg): +-mu or 0, exact
  __shared__ uint8_t sMask[64];                                // per (step, leg): the mask used
  __shared__ double sBuf[3 * 12 * 16];                         // c_k, diag(Z'RZ), d_k per step
  __shared__ double sP[144];                                   // P_k as computed (not yet mirrored)
  __shared__ __attribute__((aligned(16))) double sGY[12 * 26 + 12 * 14];  // [G | rhs], [Kp | kp kp']
  __shared__ __attribute__((aligned(16))) float sGw[24 * 16];  // gw: states, then forces
  __shared__ double sNu[2][24];                                // (nu_k, dnu_k), two steps
  double* const sCv = sBuf;
  double* const sD = sBuf + 192;
  double* const sDv = sBuf + 384;
  double* const sGM = sGY;
  double* const sY = sGY + 12 * 26;
  // arrays that live only outside the recursion share its buffers: w's forces (read by the face
  // classification) and the trajectories x_0..x_N, u_k, dx_0..dx_N, du_k of the passes after it
  float* const sU = reinterpret_cast<float*>(sGM);
  double* const sX = sBuf;
  double* const sUu = sBuf + 204;
  double* const sDX = sGY;
  double* const sDU = sGY + 204;
  extern __shared__ double sK[];  // N slots of (K_k [12][12], kappa_k [12], kappa'_k [12])
  const int lane = threadIdx.x;
  const int N = a.p.N;
  const bool need_co = a.g_x0 || a.g_gd || a.g_Ad || a.g_Bd || a.g_mu || a.g_fz;
  const GainLds s{sZx, sZy, sCv, sD, sDv, sP, sGM, sY, sK, sGw};

  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    // ---- stage the instance: the problem's loads, then the given faces, the forces (xref where
    // w is absent: read and dropped) and gw, all issued before the first LDS write waits for one
    const ProblemLoads ld = problem_issue(a.p, b, lane);
    const HeldLoads hl = held_issue(a, ld, b);
    const int eW0 = min(lane, 6 * N - 1), eW1 = min(lane + 64, 6 * N - 1);
    const float4* const gG = reinterpret_cast<const float4*>(a.gw + b * N * 24);
    const float4 vW0 = gG[eW0], vW1 = gG[eW1];
    problem_commit(sp, ld);
    reinterpret_cast<float4*>(sU)[ld.eX] = hl.vU;
    reinterpret_cast<float4*>(sGw)[eW0] = vW0;
    reinterpret_cast<float4*>(sGw)[eW1] = vW1;
    const ProblemConsts pc = problem_consts(a.p, sp, ld);
    const double mu = pc.mu;
    __syncthreads();
    const float* const sGwU = sGw + 12 * N;

    // ---- one lane per (step, leg): the mask, then its affine set
    bool ok = true;
    if (lane < 4 * N) {
      const bool stance = sC[(lane & 3) * N + (lane >> 2)] != 0;
      unsigned mask = 0;
      if (stance) mask = held_mask(a, hl, sU, lane, pc);
      sMask[lane] = (uint8_t)mask;
      ok = gain_leg_fill(sp, s, lane, mask, stance, pc);
    }
    // an inconsistent mask or an invalid entry: NaN in every output; the same decision in every
    // lane
    if (__any(!ok) || !pc.valid) {
      const double nan = __builtin_nan("");
      if (lane < 12) {
        if (a.g_x0) a.g_x0[b * 12 + lane] = nan;
        if (a.g_gd) a.g_gd[b * 12 + lane] = nan;
        if (a.g_Q) a.g_Q[b * 12 + lane] = nan;
        if (a.g_R) a.g_R[b * 12 + lane] = nan;
      }
      if (lane == 0) {
        if (a.g_mu) a.g_mu[b] = nan;
        if (a.g_fz) a.g_fz[b] = nan;
      }
      if (a.g_xref)
        for (int e = lane; e < 12 * N; e += 64) a.g_xref[b * 12 * N + e] = nan;
      if (a.g_Ad)
        for (int e = lane; e < 144; e += 64) a.g_Ad[b * 144 + e] = nan;
      if (a.g_Bd)
        for (int e = lane; e < 144 * N; e += 64) a.g_Bd[b * 144 * N + e] = nan;
      __syncthreads();
      continue;
    }

    // ---- the affine terms, then the backward Riccati recursion with the adjoint's column, then
    // the forward pass: lanes 0..11 the primal (x_k, u_k), lanes 32..43 the adjoint (dx_k, du_k)
    gain_affine(sp, s, N, lane);
    double qreg[3];  // (q_0, q'_0: not used)
    gain_recursion<2>(sp, s, N, 1, lane, qreg);
    gain_rollout<true>(sp, sK, GainTraj{sX, sUu, sDX, sDU}, N, lane);
    const int half = lane >> 5, li = lane & 31, l12 = min(li, 11);

    // ---- the outputs the trajectories give
    if (a.g_xref)
      for (int e = lane; e < 12 * N; e += 64)
        a.g_xref[b * 12 * N + e] = -2.0 * sQ[e % 12] * sDX[12 + e];
    if (lane < 12) {
      if (a.g_Q) {
        double acc = 0.0;
        for (int k = 0; k < N; ++k)
          acc = fma(sDX[(k + 1) * 12 + lane], sX[(k + 1) * 12 + lane] - (double)sXr[k * 12 + lane], acc);
        a.g_Q[b * 12 + lane] = 2.0 * acc;
      }
      if (a.g_R) {
        double acc = 0.0;
        for (int k = 0; k < N; ++k) acc = fma(sDU[k * 12 + lane], sUu[k * 12 + lane], acc);
        a.g_R[b * 12 + lane] = 2.0 * acc;
      }
    }

    // ---- backward costate pass, the outputs formed as nu_k, dnu_k are produced
    if (need_co) {
      if (li < 12) sNu[N & 1][12 * half + li] = 0.0;
      __syncthreads();
      double gAd[3] = {0.0, 0.0, 0.0}, ggd = 0.0, gmu = 0.0, gfz = 0.0;
      for (int k = N - 1; k >= 0; --k) {
        const double* const nx = sNu[(k + 1) & 1] + 12 * half;
        double* const nk = sNu[k & 1];
        if (li < 12) {
          double acc = half ? -(double)sGw[k * 12 + li]
                            : 2.0 * sQ[li] * ((double)sXr[k * 12 + li] - sX[(k + 1) * 12 + li]);
          if (half) acc = fma(-2.0 * sQ[li], sDX[(k + 1) * 12 + li], acc);
#pragma unroll
          for (int m = 0; m < 12; ++m) acc = fma((double)sAd[m * 12 + li], nx[m], acc);
          nk[12 * half + li] = acc;
        }
        __syncthreads();
        const double* const xk = sX + k * 12;
        const double* const dxk = sDX + k * 12;
        const double* const uk = sUu + k * 12;
        const double* const duk = sDU + k * 12;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const int e = min(lane + 64 * t, 143), i = e / 12, j = e - 12 * i;
          gAd[t] = fma(-nk[i], dxk[j], gAd[t]);
          gAd[t] = fma(-nk[12 + i], xk[j], gAd[t]);
          if (a.g_Bd && lane + 64 * t < 144)
            a.g_Bd[(b * N + k) * 144 + e] = -fma(nk[i], duk[j], nk[12 + i] * uk[j]);
        }
        ggd -= nk[12 + l12];
        if ((a.g_mu || a.g_fz) && lane < 4 && sC[lane * N + k] != 0) {
          const unsigned m = sMask[k * 4 + lane];
          const bool pz = m & 1u, xp = m & 2u, xn = m & 4u, yp = m & 8u, yn = m & 16u;
          if (!((xp && xn) || (yp && yn)) && m != 0) {
            // the leg's stationarity residuals: r = 2R u - Bd_k' nu, r' = 2R du + gw_u - Bd_k' dnu
            double r[3], ra[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) {
              const int j = 3 * lane + x;
              double p_ = 2.0 * sR[j] * uk[j];
              double q_ = fma(2.0 * sR[j], duk[j], (double)sGwU[k * 12 + j]);
#pragma unroll
              for (int i = 0; i < 12; ++i) {
                const double bij = (double)sBd[(k * 12 + i) * 12 + j];
                p_ = fma(-bij, nk[i], p_);
                q_ = fma(-bij, nk[12 + i], q_);
              }
              r[x] = p_, ra[x] = q_;
            }
            const double sx = xp ? 1.0 : (xn ? -1.0 : 0.0), sy = yp ? 1.0 : (yn ? -1.0 : 0.0);
            const double fz = uk[3 * lane + 2], dfz = duk[3 * lane + 2];
            gmu = fma(sx, fma(r[0], dfz, ra[0] * fz), gmu);
            gmu = fma(sy, fma(r[1], dfz, ra[1] * fz), gmu);
            if (pz) gfz += fma(sx * mu, ra[0], fma(sy * mu, ra[1], ra[2]));
          }
        }
      }
      // (the last step's barrier stands between dnu_0's write and these reads)
      if (a.g_Ad) {
#pragma unroll
        for (int t = 0; t < 3; ++t)
          if (lane + 64 * t < 144) a.g_Ad[b * 144 + lane + 64 * t] = gAd[t];
      }
      if (lane < 12) {
        if (a.g_gd) a.g_gd[b * 12 + lane] = ggd;
        if (a.g_x0) {
          double acc = 0.0;
#pragma unroll
          for (int i = 0; i < 12; ++i) acc = fma(-(double)sAd[i * 12 + lane], sNu[0][12 + i], acc);
          a.g_x0[b * 12 + lane] = acc;
        }
      }
      if (a.g_mu || a.g_fz) {  // the four legs' sums, in leg order
        const double tm = ((gain_bcast(gmu, 0) + gain_bcast(gmu, 1)) + gain_bcast(gmu, 2)) + gain_bcast(gmu, 3);
        const double tf = ((gain_bcast(gfz, 0) + gain_bcast(gfz, 1)) + gain_bcast(gfz, 2)) + gain_bcast(gfz, 3);
        if (lane == 0) {
          if (a.g_mu) a.g_mu[b] = tm;
          if (a.g_fz) a.g_fz[b] = tf;
        }
      }
    }
    __syncthreads();  // the next instance overwrites the staged arrays
  }
}

}  // namespace cmpc
