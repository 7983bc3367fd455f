// cmpc_jvp.hip -- forward-mode derivatives of the optimum on the held faces of a batch of solved
// instances: given a change d_theta of (x0, xref, gd, Q, R, mu, fz_min, Ad, Bd), the change dw of
// the whole answer (cmpc_jvp_run, include/cmpc.h).
//
// The function differentiated is cmpc_gain.hip's and cmpc_vjp.hip's: w*(theta) minimises the LQ
// problem over the forces f = Z p + c that stay on the held faces.  Its tangent solves the same
// KKT matrix with another right-hand side, so it is the same LQ problem (the same P_k, K_k) with
// other linear terms, in the halved scaling of cmpc_lq.h (cost x'Qx + u'Ru, s and r enter as
// 2 s'x and 2 r'u):
//   start          dx_0 = d_x0
//   offsets        e_k = d_gd + d_Ad x_k + d_Bd_k u_k
//   state term     on dx_{k+1}:  d_Q o (x_{k+1} - xref_k) - Q o d_xref_k - d_Ad' nu_{k+1} / 2
//   force term     on du_k:      d_R o u_k - d_Bd_k' nu_k / 2 + R o dc_k, and on the fz entry of a
//                  leg whose fz is free and which holds a friction face
//                  d_mu (sx rho_x + sy rho_y) / 2,  rho = 2R u_k - Bd_k' nu_k  (this is dZ' rho:
//                  the stationarity Z' rho = 0 differentiated in mu; -rho_x is that face's
//                  multiplier, as in cmpc_vjp.hip)
//   face offsets   dc_k = d c / d(mu, fz_min): (sx, sy, 0) d_mu fz on a leg whose fz is free,
//                  (sx t, sy t, d_fz_min) with t = d_mu fz_min + mu d_fz_min on a leg pinned at
//                  fz_min, 0 on a swing leg and on a leg that holds both signs of an axis
// with nu_k = Ad' nu_{k+1} - 2Q (x_{k+1} - xref_k), nu_N = 0, the costates of cmpc_vjp.hip.  These
// terms need the primal (x, u, nu), so the tangent cannot ride beside the primal as the adjoint
// does: the kernel runs the recursion for the primal, its forward pass and (for d_Ad, d_Bd, d_mu
// only) the costate pass, forms the terms in LDS, runs the recursion again with them in column
// 12 (gain_recursion<1, true>) and rolls the tangent out from d_x0.  Where only d_x0, d_xref,
// d_gd, d_fz_min are given no term needs the primal and the first recursion is skipped.
//
// One 64-lane wave per instance, fp64 on the fp32 inputs widened exactly, the instance staged by
// cmpc_problem.h.  The tangents are read where the terms are formed, each element once or twice,
// straight from global memory: staged, d_Bd alone would cost the wave per CU that 4n's table
// prices.  Every sum runs in an order the code fixes: bitwise repeatable, independent of B and of
// the instance's place in the batch.  Plain stores, no atomics, no workspace.
//
// This file is compiled as part of cmpc_host.hip (single translation unit).
#include "cmpc_lq.h"

namespace cmpc {

struct JvpArgs : HeldArgs {
  const float *d_x0, *d_xref, *d_gd, *d_Q, *d_R, *d_mu, *d_fz, *d_Ad, *d_Bd;  // all nullable
  double* dw;  // [B][24N]
};

__global__ void __launch_bounds__(64) jvp_kernel(JvpArgs a, int64_t B) {
  __shared__ ProblemLds sp;
  auto& [sBd, sAd, sXr, sGX, sQ, sR, sC] = sp;
  __shared__ float sZx[64], sZy[64];                           // per (step, leg): +-mu or 0, exact
  __shared__ double sCv[12 * 16], sD[12 * 16], sDv[12 * 16];   // c_k, diag(Z'RZ), d_k per step
  __shared__ double sP[144];                                   // P_k as computed (not yet mirrored)
  __shared__ __attribute__((aligned(16))) double sGM[12 * 25];  // [G | rhs]
  __shared__ double sY[12 * 13];                               // [Kp | kp]
  __shared__ double sX[12 * 17], sUu[12 * 16], sNu[12 * 17];   // x_0..x_N, u_k, nu_0..nu_N
  __shared__ double sTs[12 * 16], sTr[12 * 16], sTe[12 * 16];  // the tangent's terms per step
  // arrays that live only outside the recursion share its buffers: w's forces (read by the face
  // classification) and the tangent's forward pass dx_k, du_k
  float* const sU = reinterpret_cast<float*>(sGM);
  double* const sdx = sY;
  double* const sdu = sY + 12;
  extern __shared__ double sK[];  // N slots of (K_k [12][12], kappa_k [12])
  const int lane = threadIdx.x;
  const int N = a.p.N;
  const bool need_co = a.d_Ad || a.d_Bd || a.d_mu;
  const bool need_primal = need_co || a.d_Q || a.d_R;
  const GainLds s{sZx, sZy, sCv, sD, sDv, sP, sGM, sY, sK, nullptr, sTs, sTr, sTe};

  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    // ---- stage the instance: the problem's loads, then the given faces and the forces
    // (held_issue), all issued before the first LDS write waits for one
    const ProblemLoads ld = problem_issue(a.p, b, lane);
    const HeldLoads hl = held_issue(a, ld, b);
    problem_commit(sp, ld);
    reinterpret_cast<float4*>(sU)[ld.eX] = hl.vU;
    const ProblemConsts pc = problem_consts(a.p, sp, ld);
    __syncthreads();
    double* const dw = a.dw + b * N * 24;

    // ---- one lane per (step, leg): the mask, then its affine set
    bool ok = true, stance = false;
    unsigned mask = 0;
    if (lane < 4 * N) {
      stance = sC[(lane & 3) * N + (lane >> 2)] != 0;
      if (stance) mask = held_mask(a, hl, sU, lane, pc);
      ok = gain_leg_fill(sp, s, lane, mask, stance, pc);
    }
    // an inconsistent mask or an invalid entry: NaN in the whole row; the same decision in every
    // lane
    if (__any(!ok) || !pc.valid) {
      for (int e = lane; e < 24 * N; e += 64) dw[e] = __builtin_nan("");
      __syncthreads();
      continue;
    }
    double qreg[3];  // (q_0: not used)

    // ---- the primal: its affine terms, the recursion, the forward pass, the costates
    if (need_primal) {
      gain_affine(sp, s, N, lane);
      gain_recursion<1>(sp, s, N, 1, lane, qreg);
      gain_rollout<false>(sp, sK, GainTraj{sX, sUu, nullptr, nullptr}, N, lane);
    } else {
      __syncthreads();  // (the sets of every lane are written)
    }
    if (need_co) {
      if (lane < 12) sNu[N * 12 + lane] = 0.0;
      __syncthreads();
      for (int k = N - 1; k >= 0; --k) {
        if (lane < 12) {
          double acc = 2.0 * sQ[lane] * ((double)sXr[k * 12 + lane] - sX[(k + 1) * 12 + lane]);
#pragma unroll
          for (int m = 0; m < 12; ++m) acc = fma((double)sAd[m * 12 + lane], sNu[(k + 1) * 12 + m], acc);
          sNu[k * 12 + lane] = acc;
        }
        __syncthreads();
      }
    }

    // ---- the tangent's terms.  First per (step, entry): e_k, the state term, the force term
    // without the faces' part
    const float* const tA = a.d_Ad ? a.d_Ad + b * 144 : nullptr;
    const float* const tB = a.d_Bd ? a.d_Bd + b * N * 144 : nullptr;
    for (int e = lane; e < 12 * N; e += 64) {
      const int k = e / 12, i = e - 12 * k;
      const double* const xk = sX + k * 12;
      const double* const uk = sUu + k * 12;
      double te = a.d_gd ? (double)a.d_gd[b * 12 + i] : 0.0, ts = 0.0, tr = 0.0;
      if (a.d_Q) ts = (double)a.d_Q[b * 12 + i] * (xk[12 + i] - (double)sXr[e]);
      if (a.d_xref) ts = fma(-sQ[i], (double)a.d_xref[b * N * 12 + e], ts);
      if (a.d_R) tr = (double)a.d_R[b * 12 + i] * uk[i];
      if (tA) {
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < 12; ++m) {
          te = fma((double)tA[i * 12 + m], xk[m], te);
          acc = fma((double)tA[m * 12 + i], sNu[(k + 1) * 12 + m], acc);
        }
        ts = fma(-0.5, acc, ts);
      }
      if (tB) {
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < 12; ++m) {
          te = fma((double)tB[e * 12 + m], uk[m], te);
          acc = fma((double)tB[(k * 12 + m) * 12 + i], sNu[k * 12 + m], acc);
        }
        tr = fma(-0.5, acc, tr);
      }
      sTe[e] = te, sTs[e] = ts, sTr[e] = tr;
    }
    __syncthreads();
    // then per (step, leg): dc_k and what the faces add to the force term
    if (lane < 4 * N) {
      const int k = lane >> 2, leg = lane & 3;
      const bool pz = mask & 1u, xp = mask & 2u, xn = mask & 4u, yp = mask & 8u, yn = mask & 16u;
      double dc[3] = {0.0, 0.0, 0.0}, rz = 0.0;
      if (stance && !((xp && xn) || (yp && yn))) {
        const double sx = xp ? 1.0 : (xn ? -1.0 : 0.0), sy = yp ? 1.0 : (yn ? -1.0 : 0.0);
        const double dmu = a.d_mu ? (double)a.d_mu[b] : 0.0;
        if (pz) {
          const double dfz = a.d_fz ? (double)a.d_fz[b] : 0.0;
          const double t = fma(dmu, pc.fz_min, pc.mu * dfz);
          dc[0] = sx * t, dc[1] = sy * t, dc[2] = dfz;
        } else if (a.d_mu && (xp || xn || yp || yn)) {
          const double* const uk = sUu + k * 12;
          const double fz = uk[3 * leg + 2];
          dc[0] = sx * (dmu * fz), dc[1] = sy * (dmu * fz);
          // rho = 2R u_k - Bd_k' nu_k of the leg's x and y entries
          const int jx = 3 * leg, jy = 3 * leg + 1;
          double px = 2.0 * sR[jx] * uk[jx], py = 2.0 * sR[jy] * uk[jy];
#pragma unroll
          for (int i = 0; i < 12; ++i) {
            px = fma(-(double)sBd[(k * 12 + i) * 12 + jx], sNu[k * 12 + i], px);
            py = fma(-(double)sBd[(k * 12 + i) * 12 + jy], sNu[k * 12 + i], py);
          }
          rz = 0.5 * dmu * fma(sx, px, sy * py);
        }
      }
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        sCv[lane * 3 + x] = dc[x];
        sTr[lane * 3 + x] = fma(sR[3 * leg + x], dc[x], sTr[lane * 3 + x]) + (x == 2 ? rz : 0.0);
      }
    }
    __syncthreads();
    // then d'_k = Bd_k dc_k + e_k of every step and P_N = 0, as gain_affine does for the primal
    for (int e = lane; e < 12 * N; e += 64) {
      const int k = e / 12;
      double acc = sTe[e];
#pragma unroll
      for (int m = 0; m < 12; ++m) acc = fma((double)sBd[e * 12 + m], sCv[k * 12 + m], acc);
      sDv[e] = acc;
    }
    for (int e = lane; e < 144; e += 64) sP[e] = 0.0;
    __syncthreads();

    // ---- the recursion again with the tangent in column 12: the same K_k, the tangent's kappa_k
    gain_recursion<1, true>(sp, s, N, 1, lane, qreg);

    // ---- the tangent's forward pass from d_x0, streamed to dw: states, then forces
    if (lane < 12) sdx[lane] = a.d_x0 ? (double)a.d_x0[b * 12 + lane] : 0.0;
    __syncthreads();
    for (int k = 0; k < N; ++k) {
      const double* const Kk = sK + k * kGainSlot;
      if (lane < 12) {
        double acc = Kk[144 + lane];
#pragma unroll
        for (int m = 0; m < 12; ++m) acc = fma(Kk[lane * 12 + m], sdx[m], acc);
        sdu[lane] = acc;
        dw[(N + k) * 12 + lane] = acc;
      }
      __syncthreads();
      double xn = 0.0;
      if (lane < 12) {
        xn = sTe[k * 12 + lane];
#pragma unroll
        for (int m = 0; m < 12; ++m) xn = fma((double)sAd[lane * 12 + m], sdx[m], xn);
#pragma unroll
        for (int m = 0; m < 12; ++m) xn = fma((double)sBd[(k * 12 + lane) * 12 + m], sdu[m], xn);
        dw[k * 12 + lane] = xn;
      }
      __syncthreads();
      if (lane < 12) sdx[lane] = xn;
      __syncthreads();
    }
    __syncthreads();  // the next instance overwrites the staged arrays
  }
}

}  // namespace cmpc
