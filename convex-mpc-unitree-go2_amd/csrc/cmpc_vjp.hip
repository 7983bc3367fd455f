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
// This file is compiled as part of cmpc_host.hip (single translation unit), after cmpc_gain.hip,
// whose device helpers (gain_leg_set, gain_mm, gain_bcast, gain_rcp) it uses as they are.
#include "cmpc_problem.h"

namespace cmpc {

struct VjpArgs {
  ProblemArgs p;
  const float* w;        // nullable: its forces' faces by face_rule with p.tol
  const uint8_t* faces;  // nullable
  const float* gw;       // [B][24N]
  double *g_x0, *g_xref, *g_gd, *g_Q, *g_R, *g_mu, *g_fz, *g_Ad, *g_Bd;  // all nullable
};

constexpr int kVjpSlot = 168;  // doubles of one (K_k, kappa_k, kappa'_k) slot in LDS

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

  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    // ---- stage the instance: the problem's loads, then the given faces, the forces (xref where
    // w is absent: read and dropped) and gw, all issued before the first LDS write waits for one
    const ProblemLoads ld = problem_issue(a.p, b, lane);
    const uint8_t fgiven = (a.faces ? a.faces : a.p.contact)[b * N * 4 + ld.eC];
    const float4 vU = (a.w ? reinterpret_cast<const float4*>(a.w + b * N * 24 + 12 * N)
                           : reinterpret_cast<const float4*>(a.p.xref + b * N * 12))[ld.eX];
    const int eW0 = min(lane, 6 * N - 1), eW1 = min(lane + 64, 6 * N - 1);
    const float4* const gG = reinterpret_cast<const float4*>(a.gw + b * N * 24);
    const float4 vW0 = gG[eW0], vW1 = gG[eW1];
    problem_commit(sp, ld);
    reinterpret_cast<float4*>(sU)[ld.eX] = vU;
    reinterpret_cast<float4*>(sGw)[eW0] = vW0;
    reinterpret_cast<float4*>(sGw)[eW1] = vW1;
    const ProblemConsts pc = problem_consts(a.p, sp, ld);
    const double mu = pc.mu, fz_min = pc.fz_min;
    __syncthreads();
    const float* const sGwU = sGw + 12 * N;

    // ---- one lane per (step, leg): the mask, then its affine set
    bool ok = true;
    if (lane < 4 * N) {
      const int k = lane >> 2, leg = lane & 3;
      const bool stance = sC[leg * N + k] != 0;
      unsigned mask = 0;
      if (stance)
        mask = a.faces ? (fgiven & 31u)
                       : face_rule((double)sU[k * 12 + 3 * leg], (double)sU[k * 12 + 3 * leg + 1],
                                   (double)sU[k * 12 + 3 * leg + 2], mu, fz_min, a.p.tol);
      bool fr[3];
      double zx, zy, c[3];
      ok = gain_leg_set(mask, mu, fz_min, fr, zx, zy, c);
      if (!stance) fr[0] = fr[1] = fr[2] = false;  // f = 0: zx = zy = c = 0 already (mask 0)
      const double rx = sR[3 * leg], ry = sR[3 * leg + 1], rz = sR[3 * leg + 2];
      sZx[lane] = (float)zx;
      sZy[lane] = (float)zy;
      sMask[lane] = (uint8_t)mask;
      sCv[lane * 3] = c[0];
      sCv[lane * 3 + 1] = c[1];
      sCv[lane * 3 + 2] = c[2];
      sD[lane * 3] = fr[0] ? rx : 0.0;
      sD[lane * 3 + 1] = fr[1] ? ry : 0.0;
      sD[lane * 3 + 2] = fr[2] ? fma(zx * zx, rx, fma(zy * zy, ry, rz)) : 0.0;
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

    // d_k = Bd_k c_k + gd of every step, off the serial chain
    __syncthreads();
    for (int e = lane; e < 12 * N; e += 64) {
      const int k = e / 12, i = e - 12 * k;
      double acc = (double)sGX[i];
#pragma unroll
      for (int m = 0; m < 12; ++m) acc = fma((double)sBd[e * 12 + m], sCv[k * 12 + m], acc);
      sDv[e] = acc;
    }
    for (int e = lane; e < 144; e += 64) sP[e] = 0.0;
    __syncthreads();

    // ---- backward Riccati recursion on the f64 matrix cores, in gain_kernel's layout: lane
    // (c, g) = (lane & 15, lane >> 4) holds X[4q + g][c] of a 12x12 matrix padded to 16x16.
    // Column 12 of the B side carries the primal affine part (d, s, kappa, q), column 13 the
    // adjoint's (0, s', kappa', q').
    const int c = lane & 15, g = lane >> 4;
    const int cl = min(c, 11), cleg = cl / 3, cax = cl - 3 * cleg;
    double adg[3], qreg[3] = {0.0, 0.0, 0.0};  // [Ad | gd | 0]; q_{k+1}, q'_{k+1} on lanes c == 12, 13
#pragma unroll
    for (int q_ = 0; q_ < 3; ++q_) {
      const int rq = 4 * q_ + g;
      adg[q_] = c < 12 ? (double)sAd[rq * 12 + c] : (c == 12 ? (double)sGX[rq] : 0.0);
    }
    for (int k = N - 1; k >= 0; --k) {
      const float* const Bk = sBd + k * 144;
      const double* const Dk = sD + k * 12;
      double* const Kk = sK + k * kVjpSlot;
      const bool used = c < 12 && Dk[cl] != 0.0;
      double sa[3], bt[3], wv[3], ab[3], sreg[3], rb[3];
#pragma unroll
      for (int q_ = 0; q_ < 3; ++q_) {
        const int rq = 4 * q_ + g;
        // S = Q + P_{k+1}, mirrored here: A operand S[c][rq]
        const double sym = 0.5 * (sP[cl * 12 + rq] + sP[rq * 12 + cl]) + (cl == rq ? sQ[cl] : 0.0);
        sa[q_] = c < 12 ? sym : 0.0;
        // Bt = Bd_k Z: column c is slot c of leg cleg
        const float* const bi = Bk + rq * 12 + 3 * cleg;
        const double v = cax == 2 ? fma((double)sZx[k * 4 + cleg], (double)bi[0],
                                        fma((double)sZy[k * 4 + cleg], (double)bi[1], (double)bi[2]))
                                  : (double)bi[cax];
        bt[q_] = used ? v : 0.0;
        wv[q_] = c == 12 ? sDv[k * 12 + rq] : adg[q_];  // [Ad | d_k | 0], 0 past column 12
        ab[q_] = c < 12 ? (double)Bk[cl * 12 + rq] : 0.0;  // A operand Bd_k[c][rq]
        // s on lanes c == 12, s' on lanes c == 13
        sreg[q_] = c == 13 ? fma(0.5, (double)sGw[k * 12 + rq], qreg[q_])
                           : qreg[q_] - sQ[rq] * (double)sXr[k * 12 + rq];
        rb[q_] = c == 13 ? 0.5 * (double)sGwU[k * 12 + rq] : 0.0;  // r = gw_u,k / 2 in column 13
      }
      const gain_d4 zero = {0.0, 0.0, 0.0, 0.0};
      gain_d4 SW = gain_mm(sa, wv, zero);  // [S Ad | S d | 0]
      gain_d4 SB = gain_mm(sa, bt, zero);  // S Bt
      double swb[3], sbb[3];
      const bool aff = c == 12 || c == 13;
#pragma unroll
      for (int r_ = 0; r_ < 3; ++r_) {
        swb[r_] = aff ? SW[r_] + sreg[r_] : SW[r_];  // columns 12, 13: S d + s, s'
        sbb[r_] = SB[r_];
      }
      gain_d4 G = gain_mm(bt, sbb, zero);  // Bt'S Bt
      gain_d4 M = gain_mm(bt, swb, zero);  // [Bt'S Ad | Bt'(S d + s) | Bt's']
      // [G | M] to LDS, G = Bt'S Bt + D with 1 on the diagonal of a slot not in use; column 13
      // of M takes Z'r on the slots in use
      if (c < 14) {
#pragma unroll
        for (int r_ = 0; r_ < 3; ++r_) {
          const int i = g + 4 * r_, leg = i / 3, ax = i - 3 * leg;
          if (c < 12) sGM[i * 26 + c] = c == i ? G[r_] + (Dk[i] != 0.0 ? Dk[i] : 1.0) : G[r_];
          double m = M[r_];
          if (c == 13 && Dk[i] != 0.0) {
            const float* const ru = sGwU + k * 12 + 3 * leg;
            const double zr = ax == 2 ? fma((double)sZx[k * 4 + leg], (double)ru[0],
                                            fma((double)sZy[k * 4 + leg], (double)ru[1], (double)ru[2]))
                                      : (double)ru[ax];
            m = fma(0.5, zr, m);
          }
          sGM[i * 26 + 12 + c] = m;
        }
      }
      __syncthreads();
      // eliminate, one column per lane (lanes past 25 repeat column 25), then back-substitute the
      // 14 right-hand sides on lanes 12..25, column by column
      {
        const int cc = min(lane, 25);
        double col[12], rp[12], y[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) col[i] = sGM[i * 26 + cc];
#pragma unroll
        for (int j = 0; j < 12; ++j) {
          rp[j] = gain_rcp(gain_bcast(col[j], j));
#pragma unroll
          for (int i = j + 1; i < 12; ++i) {
            const double mij = gain_bcast(col[i], j) * rp[j];
            col[i] = fma(-mij, col[j], col[i]);
          }
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) y[i] = col[i];
#pragma unroll
        for (int j = 11; j >= 0; --j) {
          y[j] *= rp[j];
#pragma unroll
          for (int i = 0; i < j; ++i) y[i] = fma(-gain_bcast(col[i], j), y[j], y[i]);
        }
        if (lane >= 12 && lane < 26) {
#pragma unroll
          for (int i = 0; i < 12; ++i) sY[i * 14 + lane - 12] = -y[i];
        }
      }
      __syncthreads();
      // [K_k | kappa_k | kappa'_k] = Z [Kp | kp | kp'] + [0 | c_k | 0] as a B operand; kept in LDS
      double kb[3], ka[3], kpb[3], kt[3];
      const int c14 = min(c, 13);
#pragma unroll
      for (int q_ = 0; q_ < 3; ++q_) {
        const int rq = 4 * q_ + g, leg = rq / 3, ax = rq - 3 * leg;
        const double yv = sY[rq * 14 + c14];
        double v = yv;
        if (ax < 2)
          v = fma((double)(ax == 0 ? sZx[k * 4 + leg] : sZy[k * 4 + leg]),
                  sY[(3 * leg + 2) * 14 + c14], v);
        if (c == 12) v += sCv[k * 12 + rq];
        kb[q_] = c < 14 ? v : 0.0;
        kpb[q_] = c < 14 ? yv : 0.0;
        ka[q_] = c < 12 ? yv * Dk[rq] : 0.0;
        kt[q_] = c < 12 ? v : 0.0;  // A operand K_k'
        if (c < 12) Kk[rq * 12 + c] = v;
        else if (c < 14) Kk[144 + 12 * (c - 12) + rq] = v;
      }
      const gain_d4 ad0 = {adg[0], adg[1], adg[2], 0.0};
      gain_d4 AC = gain_mm(ab, kb, ad0);  // [A_cl | d_cl | d'_cl] = [Ad | gd | 0] + Bd_k [K_k | kappa_k | kappa'_k]
      double acb[3], sacb[3];
#pragma unroll
      for (int r_ = 0; r_ < 3; ++r_) acb[r_] = AC[r_];
      gain_d4 SAC = gain_mm(sa, acb, zero);  // [S A_cl | S d_cl | S d'_cl]
#pragma unroll
      for (int r_ = 0; r_ < 3; ++r_) sacb[r_] = aff ? SAC[r_] + sreg[r_] : SAC[r_];
      gain_d4 Pn = gain_mm(acb, sacb, zero);  // [A_cl'S A_cl | A_cl'(S d_cl + s) | A_cl'(S d'_cl + s')]
      Pn = gain_mm(ka, kpb, Pn);              // + [Kp'D Kp | Kp'D kp | Kp'D kp']
      Pn = gain_mm(kt, rb, Pn);               // + [0 | 0 | K_k'r]
#pragma unroll
      for (int r_ = 0; r_ < 3; ++r_) {
        if (c < 12) sP[(g + 4 * r_) * 12 + c] = Pn[r_];
        qreg[r_] = Pn[r_];  // q_k, q'_k on lanes c == 12, 13
      }
      __syncthreads();
    }

    // ---- forward pass: lanes 0..11 the primal (x_k, u_k), lanes 32..43 the adjoint (dx_k, du_k)
    const int half = lane >> 5, li = lane & 31, l12 = min(li, 11);
    double* const tx = half ? sDX : sX;
    double* const tu = half ? sDU : sUu;
    if (li < 12) tx[li] = half ? 0.0 : (double)sGX[12 + li];
    __syncthreads();
    for (int k = 0; k < N; ++k) {
      const double* const Kk = sK + k * kVjpSlot;
      if (li < 12) {
        double acc = Kk[144 + 12 * half + li];
#pragma unroll
        for (int m = 0; m < 12; ++m) acc = fma(Kk[li * 12 + m], tx[k * 12 + m], acc);
        tu[k * 12 + li] = acc;
      }
      __syncthreads();
      if (li < 12) {
        double xn = half ? 0.0 : (double)sGX[li];
#pragma unroll
        for (int m = 0; m < 12; ++m) xn = fma((double)sAd[li * 12 + m], tx[k * 12 + m], xn);
#pragma unroll
        for (int m = 0; m < 12; ++m) xn = fma((double)sBd[(k * 12 + li) * 12 + m], tu[k * 12 + m], xn);
        tx[(k + 1) * 12 + li] = xn;
      }
      __syncthreads();
    }

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
