// cmpc_gain.hip -- feedback gain K = d u_0 / d x_0, value-function gradient and Hessian and the
// optimum on the held faces of a batch of solved instances (cmpc_gain_run, include/cmpc.h;
// DESIGN.md 4l).
//
// On the faces its forces hold, the QP is an equality-constrained LQ problem.  Each stance leg's
// force is f = Z p + c with the 3 parameter slots
//   slot 0: fx, free unless an fx face is held        column e_x
//   slot 1: fy, free unless an fy face is held        column e_y
//   slot 2: fz, free unless fz is pinned              column (sx mu, sy mu, 1), sx, sy the held signs
// and c the pinned part (nonzero only with fz = fz_min != 0).  A slot that is not free keeps its
// place with a zero column, so every step has 12 slots: G = Bt'S Bt + Z'RZ gets a 1 on the
// diagonal of such a slot and its row of the solve is exactly zero.  Z'RZ is diagonal and
// Z'R c = 0 because a held fx / fy enters only column 2 or c, never its own slot.
//
// Backward, from P_N = 0, q_N = 0, with S = Q + P_{k+1}, s = q_{k+1} - Q xref_k, Bt = Bd_k Z,
// d = Bd_k c + gd, D = Z'RZ:
//   [Kp | kp] = -G^-1 [Bt'S Ad | Bt'(S d + s)]        K_k = Z Kp,  kappa_k = c + Z kp
//   A_cl = Ad + Bd_k K_k,  d_cl = Bd_k kappa_k + gd
//   P_k = A_cl'S A_cl + Kp'D Kp (mirrored: (P + P')/2),  q_k = A_cl'(S d_cl + s) + Kp'D kp
// then K = K_0, Vxx = 2 P_0, Vx = 2 (P_0 x_0 + q_0) and the forward pass u_k = K_k x_k + kappa_k.
//
// One 64-lane wave per instance, fp64 on the fp32 inputs widened exactly.  The instance is
// staged in LDS by cmpc_problem.h (16-byte loads, all issued before the first is used).  The
// eight 12x12 products of a step run on the f64 matrix cores (v_mfma_f64_16x16x4_f64, three per
// product, the matrices padded to 16x16), chained from register to register: a product comes
// out in the layout the next one takes as its B operand or as a transposed A operand, and
// column 12 of the padding carries the affine part (d, s, kappa, q) through the same products.
// The solve with G is Gaussian elimination without pivoting (G is SPD) on the 25 columns
// [G | 13 right-hand sides], one column per lane in registers, the multipliers broadcast from
// the pivot's lane: no LDS traffic and no barrier inside it; it is the serial part of a step.
// Every sum runs in an order the code fixes: bitwise repeatable, independent of B and of the
// instance's place in the batch.  No atomics, no workspace.
//
// This file is compiled as part of cmpc_host.hip (single translation unit).
#include "cmpc_problem.h"

namespace cmpc {

struct GainArgs {
  ProblemArgs p;
  const float* w;        // nullable: its forces' faces by face_rule with p.tol
  const uint8_t* faces;  // nullable
  double *K, *Vx, *Vxx, *u_star;  // all but K nullable
  uint8_t* faces_out;             // nullable
};

constexpr int kGainSlot = 156;  // doubles of one (K_k, kappa_k) slot in LDS

// The affine set f = Z p + c of a stance leg's mask: free[3] the slots in use, zx / zy the x / y
// entries of slot 2's column.  false: the mask is inconsistent.
__device__ inline bool gain_leg_set(unsigned m, double mu, double fz_min, bool free_[3],
                                    double& zx, double& zy, double c[3]) {
  const bool pz = m & 1u, xp = m & 2u, xn = m & 4u, yp = m & 8u, yn = m & 16u;
  const bool both = (xp && xn) || (yp && yn);
  c[0] = c[1] = c[2] = 0.0;
  zx = zy = 0.0;
  free_[0] = !(xp || xn);
  free_[1] = !(yp || yn);
  free_[2] = !(pz || both);
  if (both && pz && fz_min != 0.0) return false;
  if (free_[2]) {
    zx = xp ? mu : (xn ? -mu : 0.0);
    zy = yp ? mu : (yn ? -mu : 0.0);
  } else {
    const double z = both ? 0.0 : fz_min;  // both signs of an axis: fz = 0
    c[0] = (xp && xn) ? 0.0 : (xp ? mu * z : (xn ? -mu * z : 0.0));
    c[1] = (yp && yn) ? 0.0 : (yp ? mu * z : (yn ? -mu * z : 0.0));
    c[2] = z;
  }
  return true;
}

typedef double gain_d4 __attribute__((ext_vector_type(4)));

// acc + A B of 12x12 matrices padded to 16x16 on v_mfma_f64_16x16x4_f64: lane (c, g) gives
// a[q] = A[c][4q + g] and b[q] = B[4q + g][c]; register r of the result is row g + 4r, column c
__device__ inline gain_d4 gain_mm(const double a[3], const double b[3], gain_d4 acc) {
#pragma unroll
  for (int q = 0; q < 3; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b[q], acc, 0, 0, 0);
  return acc;
}

// lane src's v in every lane (src is wave-uniform: two v_readlane, no LDS permute)
__device__ inline double gain_bcast(double v, int src) {
  const long long u = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)u, src);
  const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(u >> 32), src);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// 1 / x of a pivot (positive, normal): v_rcp_f64 and two Newton steps, without the scaling and
// fix-up a division carries for subnormal and infinite operands
__device__ inline double gain_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(r, fma(-x, r, 1.0), r);
  return fma(r, fma(-x, r, 1.0), r);
}

// The LDS arrays of the backward recursion next to the staged problem
struct GainLds {
  const float *Zx, *Zy;       // per (step, leg): +-mu or 0, exact
  const double *Cv, *D, *Dv;  // per step: c_k, diag(Z'RZ), d_k = Bd_k c_k + gd
  double* P;                  // [144] P_k as computed (not yet mirrored); zero (P_N) on entry
  double *GM, *Y;             // [12 * 25] [G | rhs], 16-byte aligned; [12 * 13] [Kp | kp]
  double* K;                  // keep_steps ? N : 1 slots of (K_k [12][12], kappa_k [12])
};

// The backward recursion of the header's comment over the steps N-1 .. 0 for the whole wave:
// leaves (K_k, kappa_k) in the slots of s.K, P_0 (not mirrored) in s.P and q_0 in qreg on the
// lanes with (lane & 15) == 12 (entry (lane >> 4) + 4 r in qreg[r]).  The caller's barrier
// stands before the call; the last step's barrier ends it.  gain_kernel and refine_kernel
// (cmpc_refine.hip) both run it.
__device__ __forceinline__ void gain_recursion(ProblemLds& sp, const GainLds& s, int N,
                                               int keep_steps, int lane, double qreg[3]) {
  auto& [sBd, sAd, sXr, sGX, sQ, sR, sC] = sp;
  const float *const sZx = s.Zx, *const sZy = s.Zy;
  const double *const sCv = s.Cv, *const sD = s.D, *const sDv = s.Dv;
  double *const sP = s.P, *const sGM = s.GM, *const sY = s.Y, *const sK = s.K;
  // ---- backward Riccati recursion on the f64 matrix cores.  Lane (c, g) = (lane & 15,
  // lane >> 4) holds, of a 12x12 matrix X padded to 16x16, the three entries X[4q + g][c]:
  // that is the B operand of X (pass q carries k = 4q + g), the A operand of X', and the
  // layout a product comes out in (row g + 4 reg, column c) -- so products chain from
  // register to register.  Column 12 of the B side carries the affine part (d, s, kappa, q).
  const int c = lane & 15, g = lane >> 4;
  const int cl = min(c, 11), cleg = cl / 3, cax = cl - 3 * cleg;
  double adg[3];  // [Ad | gd] in that layout; qreg: q_{k+1} on lanes c == 12
#pragma unroll
  for (int q_ = 0; q_ < 3; ++q_) {
    const int rq = 4 * q_ + g;
    adg[q_] = c < 12 ? (double)sAd[rq * 12 + c] : (c == 12 ? (double)sGX[rq] : 0.0);
    qreg[q_] = 0.0;
  }
  for (int k = N - 1; k >= 0; --k) {
    const float* const Bk = sBd + k * 144;
    const double* const Dk = sD + k * 12;
    double* const Kk = sK + (keep_steps ? k : 0) * kGainSlot;
    const bool used = c < 12 && Dk[cl] != 0.0;
    double sa[3], bt[3], wv[3], ab[3], sreg[3];
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
      wv[q_] = c == 12 ? sDv[k * 12 + rq] : adg[q_];  // [Ad | d_k], 0 past column 12
      ab[q_] = c < 12 ? (double)Bk[cl * 12 + rq] : 0.0;  // A operand Bd_k[c][rq]
      sreg[q_] = qreg[q_] - sQ[rq] * (double)sXr[k * 12 + rq];  // s, used on lanes c == 12
    }
    const gain_d4 zero = {0.0, 0.0, 0.0, 0.0};
    gain_d4 SW = gain_mm(sa, wv, zero);  // [S Ad | S d]
    gain_d4 SB = gain_mm(sa, bt, zero);  // S Bt
    double swb[3], sbb[3];
#pragma unroll
    for (int r_ = 0; r_ < 3; ++r_) {
      swb[r_] = c == 12 ? SW[r_] + sreg[r_] : SW[r_];  // column 12: S d + s
      sbb[r_] = SB[r_];
    }
    gain_d4 G = gain_mm(bt, sbb, zero);  // Bt'S Bt
    gain_d4 M = gain_mm(bt, swb, zero);  // [Bt'S Ad | Bt'(S d + s)]
    // [G | M] to LDS, G = Bt'S Bt + D with 1 on the diagonal of a slot not in use
    if (c < 13) {
#pragma unroll
      for (int r_ = 0; r_ < 3; ++r_) {
        const int i = g + 4 * r_;
        if (c < 12) sGM[i * 25 + c] = c == i ? G[r_] + (Dk[i] != 0.0 ? Dk[i] : 1.0) : G[r_];
        sGM[i * 25 + 12 + c] = M[r_];
      }
    }
    __syncthreads();
    // eliminate, one column per lane (lanes past 24 repeat column 24), then back-substitute the
    // 13 right-hand sides on lanes 12..24, column by column: once y[j] is known every row
    // above takes its term, so the dependent chain is two operations per unknown
    {
      const int cc = min(lane, 24);
      double col[12], rp[12], y[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) col[i] = sGM[i * 25 + cc];
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
      if (lane >= 12 && lane < 25) {
#pragma unroll
        for (int i = 0; i < 12; ++i) sY[i * 13 + lane - 12] = -y[i];
      }
    }
    __syncthreads();
    // [K_k | kappa_k] = Z [Kp | kp] + [0 | c_k] as a B operand; kept in LDS for the outputs
    double kb[3], ka[3], kpb[3];
    const int c13 = min(c, 12);
#pragma unroll
    for (int q_ = 0; q_ < 3; ++q_) {
      const int rq = 4 * q_ + g, leg = rq / 3, ax = rq - 3 * leg;
      const double yv = sY[rq * 13 + c13];
      double v = yv;
      if (ax < 2)
        v = fma((double)(ax == 0 ? sZx[k * 4 + leg] : sZy[k * 4 + leg]),
                sY[(3 * leg + 2) * 13 + c13], v);
      if (c == 12) v += sCv[k * 12 + rq];
      kb[q_] = c < 13 ? v : 0.0;
      kpb[q_] = c < 13 ? yv : 0.0;
      ka[q_] = c < 12 ? yv * Dk[rq] : 0.0;
      if (c < 12) Kk[rq * 12 + c] = v;
      else if (c == 12) Kk[144 + rq] = v;
    }
    const gain_d4 ad0 = {adg[0], adg[1], adg[2], 0.0};
    gain_d4 AC = gain_mm(ab, kb, ad0);  // [A_cl | d_cl] = [Ad | gd] + Bd_k [K_k | kappa_k]
    double acb[3], sacb[3];
#pragma unroll
    for (int r_ = 0; r_ < 3; ++r_) acb[r_] = AC[r_];
    gain_d4 SAC = gain_mm(sa, acb, zero);  // [S A_cl | S d_cl]
#pragma unroll
    for (int r_ = 0; r_ < 3; ++r_) sacb[r_] = c == 12 ? SAC[r_] + sreg[r_] : SAC[r_];
    gain_d4 Pn = gain_mm(acb, sacb, zero);  // [A_cl'S A_cl | A_cl'(S d_cl + s)]
    Pn = gain_mm(ka, kpb, Pn);              // + [Kp'D Kp | Kp'D kp]
#pragma unroll
    for (int r_ = 0; r_ < 3; ++r_) {
      if (c < 12) sP[(g + 4 * r_) * 12 + c] = Pn[r_];
      qreg[r_] = Pn[r_];  // q_k on lanes c == 12
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(64) gain_kernel(GainArgs a, int64_t B, int keep_steps) {
  __shared__ ProblemLds sp;
  auto& [sBd, sAd, sXr, sGX, sQ, sR, sC] = sp;
  __shared__ float sZx[64], sZy[64];                           // per (step, leg): +-mu or 0, exact
  __shared__ double sCv[12 * 16], sD[12 * 16];                 // c_k and diag(Z'RZ) per step
  __shared__ double sDv[12 * 16];                              // d_k = Bd_k c_k + gd per step
  __shared__ double sP[144], sq[12];                           // P_k as computed (not yet mirrored)
  __shared__ __attribute__((aligned(16))) double sGM[12 * 25];  // [G | rhs]
  __shared__ double sY[12 * 13];                               // [Kp | kp]
  // two arrays live only outside the recursion share its buffers: w's forces u_0..u_{N-1}
  // (read by the face classification) and the forward pass's x_k, u_k
  float* const sU = reinterpret_cast<float*>(sGM);
  double* const sx = sY;
  double* const su = sY + 12;
  extern __shared__ double sK[];  // keep_steps ? N : 1 slots of (K_k [12][12], kappa_k [12])
  const int lane = threadIdx.x;
  const int N = a.p.N;

  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    // ---- stage the instance: the problem's loads, then the given faces and the forces (xref
    // where w is absent: read and dropped), all issued before the first LDS write waits for one.
    // The faces go before the forces: they are used under a branch only, and the forces' LDS
    // write, waiting for the last load, covers them.  Pending into the next instance they make
    // the first write of their register wait for everything issued before it.
    const ProblemLoads ld = problem_issue(a.p, b, lane);
    const uint8_t fgiven = (a.faces ? a.faces : a.p.contact)[b * N * 4 + ld.eC];
    const float4 vU = (a.w ? reinterpret_cast<const float4*>(a.w + b * N * 24 + 12 * N)
                           : reinterpret_cast<const float4*>(a.p.xref + b * N * 12))[ld.eX];
    problem_commit(sp, ld);
    reinterpret_cast<float4*>(sU)[ld.eX] = vU;
    const ProblemConsts pc = problem_consts(a.p, sp, ld);
    const double mu = pc.mu, fz_min = pc.fz_min;
    __syncthreads();

    // ---- one lane per (step, leg): the mask, then its affine set
    bool ok = true;
    unsigned mask = 0;
    if (lane < 4 * N) {
      const int k = lane >> 2, leg = lane & 3;
      const bool stance = sC[leg * N + k] != 0;
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
      sCv[lane * 3] = c[0];
      sCv[lane * 3 + 1] = c[1];
      sCv[lane * 3 + 2] = c[2];
      sD[lane * 3] = fr[0] ? rx : 0.0;
      sD[lane * 3 + 1] = fr[1] ? ry : 0.0;
      sD[lane * 3 + 2] = fr[2] ? fma(zx * zx, rx, fma(zy * zy, ry, rz)) : 0.0;
    }
    // an inconsistent mask or an invalid entry: NaN in every output, 0xFF in faces_out; the same
    // decision in every lane
    if (__any(!ok) || !pc.valid) {
      const double nan = __builtin_nan("");
      for (int e = lane; e < 144; e += 64) {
        a.K[b * 144 + e] = nan;
        if (a.Vxx) a.Vxx[b * 144 + e] = nan;
      }
      if (a.Vx && lane < 12) a.Vx[b * 12 + lane] = nan;
      if (a.u_star)
        for (int e = lane; e < 12 * N; e += 64) a.u_star[b * 12 * N + e] = nan;
      if (a.faces_out && lane < 4 * N) a.faces_out[b * 4 * N + lane] = 0xFF;
      __syncthreads();
      continue;
    }
    if (a.faces_out && lane < 4 * N) a.faces_out[b * 4 * N + lane] = (uint8_t)mask;

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

    // ---- backward Riccati recursion on the f64 matrix cores (gain_recursion)
    const int c = lane & 15, g = lane >> 4;
    double qreg[3];
    gain_recursion(sp, GainLds{sZx, sZy, sCv, sD, sDv, sP, sGM, sY, sK}, N, keep_steps, lane, qreg);
    if (c == 12) {
#pragma unroll
      for (int r_ = 0; r_ < 3; ++r_) sq[g + 4 * r_] = qreg[r_];
    }
    __syncthreads();

    // ---- outputs
    for (int e = lane; e < 144; e += 64) {
      a.K[b * 144 + e] = sK[e];
      if (a.Vxx) a.Vxx[b * 144 + e] = sP[e] + sP[(e % 12) * 12 + e / 12];  // 2 x the mirrored P_0
    }
    if (a.Vx && lane < 12) {
      double acc = sq[lane];
#pragma unroll
      for (int m = 0; m < 12; ++m)
        acc = fma(0.5 * (sP[lane * 12 + m] + sP[m * 12 + lane]), (double)sGX[12 + m], acc);
      a.Vx[b * 12 + lane] = 2.0 * acc;
    }
    if (a.u_star) {  // (keep_steps is set: every K_k is in LDS)
      if (lane < 12) sx[lane] = (double)sGX[12 + lane];
      __syncthreads();
      for (int k = 0; k < N; ++k) {
        const double* const Kk = sK + k * kGainSlot;
        if (lane < 12) {
          double acc = Kk[144 + lane];
#pragma unroll
          for (int m = 0; m < 12; ++m) acc = fma(Kk[lane * 12 + m], sx[m], acc);
          su[lane] = acc;
          a.u_star[(b * N + k) * 12 + lane] = acc;
        }
        __syncthreads();
        double xn = 0.0;
        if (lane < 12) {
          xn = (double)sGX[lane];
#pragma unroll
          for (int m = 0; m < 12; ++m) xn = fma((double)sAd[lane * 12 + m], sx[m], xn);
#pragma unroll
          for (int m = 0; m < 12; ++m) xn = fma((double)sBd[(k * 12 + lane) * 12 + m], su[m], xn);
        }
        __syncthreads();
        if (lane < 12) sx[lane] = xn;
        __syncthreads();
      }
    }
    __syncthreads();  // the next instance overwrites the staged arrays
  }
}

}  // namespace cmpc
