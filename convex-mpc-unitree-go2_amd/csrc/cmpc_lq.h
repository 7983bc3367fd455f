// cmpc_lq.h -- the equality-constrained LQ problem on the faces a solved instance holds, which
// cmpc_gain.hip, cmpc_vjp.hip, cmpc_refine.hip and cmpc_jvp.hip all evaluate: the
// held-face part of their argument blocks and its two loads, the lane's mask and its affine set, the affine
// terms d_k, the backward Riccati recursion on the f64 matrix cores and the forward pass that
// keeps whole trajectories.  Included by those four files only, on top of cmpc_problem.h.  The
// masks one entry writes are the masks another reads and refine's point is gain's u_star, so
// each of these exists once.
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
// and forward u_k = K_k x_k + kappa_k, x_{k+1} = Ad x_k + Bd_k u_k + gd.  The adjoint of
// cmpc_vjp.hip is the same problem with other linear terms (s' = q'_{k+1} + gw_x,k / 2, a force
// term r = gw_u,k / 2, d' = 0) and rides along as a second affine column.
#pragma once
#include <type_traits>

#include "cmpc_problem.h"

namespace cmpc {

// the leading fields of GainArgs, VjpArgs and RefineArgs
struct HeldArgs {
  ProblemArgs p;
  const float* w;        // nullable: its forces' faces by face_rule with p.tol
  const uint8_t* faces;  // nullable
};

// what held_issue has in flight
struct HeldLoads {
  uint8_t fgiven;  // the given mask of (step, leg) eC (the contact byte where faces is absent)
  float4 vU;       // piece eX of w's forces (of xref where w is absent: read and dropped)
};

// The held-face loads of instance b, between problem_issue and problem_commit so that all of an
// instance's loads are issued before the first LDS write waits for one.  The faces go before the
// forces: they are used under a branch only, and the forces' LDS write (the caller's, at float4
// index ld.eX, after problem_commit), waiting for the last load, covers them.  Pending into the
// next instance they make the first write of their register wait for everything issued before it.
__device__ inline HeldLoads held_issue(const HeldArgs& a, const ProblemLoads& ld, int64_t b) {
  const int N = a.p.N;
  HeldLoads v;
  v.fgiven = (a.faces ? a.faces : a.p.contact)[b * N * 4 + ld.eC];
  v.vU = (a.w ? reinterpret_cast<const float4*>(a.w + b * N * 24 + 12 * N)
              : reinterpret_cast<const float4*>(a.p.xref + b * N * 12))[ld.eX];
  return v;
}

// The mask of the stance leg of lane = 4 step + leg: the given one, or by face_rule off the staged
// forces sU
__device__ inline unsigned held_mask(const HeldArgs& a, const HeldLoads& v, const float* sU,
                                     int lane, const ProblemConsts& pc) {
  const float* const f = sU + 3 * lane;  // (= step * 12 + 3 leg)
  return a.faces ? (v.fgiven & 31u)
                 : face_rule((double)f[0], (double)f[1], (double)f[2], pc.mu, pc.fz_min, a.p.tol);
}

constexpr int lq_slot(int naff) { return 144 + 12 * naff; }  // doubles of one (K_k, kappa_k ..) slot
constexpr int kGainSlot = lq_slot(1);  // (K_k, kappa_k)
constexpr int kVjpSlot = lq_slot(2);   // (K_k, kappa_k, kappa'_k)

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

// The LDS arrays of the LQ problem next to the staged one; each kernel lays out and aliases its own
struct GainLds {
  float *Zx, *Zy;       // per (step, leg): +-mu or 0, exact
  double *Cv, *D, *Dv;  // per step: c_k, diag(Z'RZ), d_k = Bd_k c_k + gd
  double* P;            // [144] P_k as computed (not yet mirrored)
  double *GM, *Y;       // [12 * (24 + NAFF)] [G | rhs], 16-byte aligned; [12 * (12 + NAFF)] [Kp | kp ..]
  double* K;            // keep_steps ? N : 1 slots of (K_k [12][12], kappa_k [12], .. NAFF of them)
  const float* Gw;      // NAFF == 2: gw [24N], states then forces
  const double *Ts, *Tr, *Te;  // TAN: per step, the state term, the force term r and the offset e_k
};

// A pointer into LDS that says so in its type: what gain_recursion<2> reads the bundle through.
// The function is compiled before it is inlined into a kernel; through plain pointers it sees
// generic addresses indexed in 64 bits, and what reaches vjp_kernel then keeps more addresses in
// registers than the same loop written in the kernel did (six AGPRs).  With one
// affine column the plain pointers stay: typed, gain_kernel measured 0.6 % slower.
template <class T> using lds_ptr = __attribute__((address_space(3))) T*;

// The affine set of the mask of lane = 4 step + leg (< 4N) to Zx, Zy, Cv, D; a leg in swing holds
// no force.  gain_leg_set's verdict.
__device__ inline bool gain_leg_fill(const ProblemLds& sp, const GainLds& s, int lane, unsigned mask,
                                    bool stance, const ProblemConsts& pc) {
  const int leg = lane & 3;
  bool fr[3];
  double zx, zy, c[3];
  const bool ok = gain_leg_set(mask, pc.mu, pc.fz_min, fr, zx, zy, c);
  if (!stance) fr[0] = fr[1] = fr[2] = false;  // f = 0: zx = zy = c = 0 already (mask 0)
  const double rx = sp.R[3 * leg], ry = sp.R[3 * leg + 1], rz = sp.R[3 * leg + 2];
  s.Zx[lane] = (float)zx;
  s.Zy[lane] = (float)zy;
  s.Cv[lane * 3] = c[0];
  s.Cv[lane * 3 + 1] = c[1];
  s.Cv[lane * 3 + 2] = c[2];
  s.D[lane * 3] = fr[0] ? rx : 0.0;
  s.D[lane * 3 + 1] = fr[1] ? ry : 0.0;
  s.D[lane * 3 + 2] = fr[2] ? fma(zx * zx, rx, fma(zy * zy, ry, rz)) : 0.0;
  return ok;
}

// d_k = Bd_k c_k + gd of every step, off the serial chain, and P_N = 0: what the recursion finds
// on entry.  A barrier stands before (the sets of every lane are written) and after.
__device__ inline void gain_affine(const ProblemLds& sp, const GainLds& s, int N, int lane) {
  __syncthreads();
  for (int e = lane; e < 12 * N; e += 64) {
    const int k = e / 12, i = e - 12 * k;
    double acc = (double)sp.GX[i];
#pragma unroll
    for (int m = 0; m < 12; ++m) acc = fma((double)sp.Bd[e * 12 + m], s.Cv[k * 12 + m], acc);
    s.Dv[e] = acc;
  }
  for (int e = lane; e < 144; e += 64) s.P[e] = 0.0;
  __syncthreads();
}

// The backward recursion of the header's comment over the steps N-1 .. 0 for the whole wave, with
// NAFF affine columns: 1 the problem's own, 2 the adjoint's next to it.  Leaves (K_k, kappa_k ..)
// in the slots of s.K, P_0 (not mirrored) in s.P and q_0 (q'_0) in qreg on the lanes with
// (lane & 15) == 12 (13), entry (lane >> 4) + 4 r in qreg[r].  The caller's barrier stands before
// the call; the last step's barrier ends it.
//
// TAN (cmpc_jvp.hip, NAFF == 1): column 12 carries a tangent problem instead of the instance's
// own, the same matrices with the general linear terms of s.Ts, s.Tr, s.Te:
//   s = q_{k+1} + Ts_k    a force term r = Tr_k (Z'r joins the solve's right-hand side, K_k'r
//   joins q_k, as the adjoint's)    x_{k+1} = Ad x_k + Bd_k u_k + Te_k
// and the caller fills s.Cv with the tangent's c_k and s.Dv with Bd_k c_k + Te_k.  Its c_k need
// not satisfy Z'R c = 0: the caller adds R c_k to Tr_k.
template <int NAFF, bool TAN = false>
__device__ __forceinline__ void gain_recursion(ProblemLds& sp, const GainLds& s, int N,
                                               int keep_steps, int lane, double qreg[3]) {
  static_assert(NAFF == 1 || NAFF == 2, "one affine column, or the adjoint's next to it");
  static_assert(!TAN || NAFF == 1, "the tangent's terms take the place of column 12");
  constexpr int GW = 24 + NAFF, YW = 12 + NAFF;  // row strides of [G | rhs] and [Kp | kp ..]
  auto& [sBd, sAd, sXr, sGX, sQ, sR, sC] = sp;
  using PF = std::conditional_t<NAFF == 2, lds_ptr<const float>, const float*>;
  using PC = std::conditional_t<NAFF == 2, lds_ptr<const double>, const double*>;
  using PD = std::conditional_t<NAFF == 2, lds_ptr<double>, double*>;
  const PF sZx = (PF)s.Zx, sZy = (PF)s.Zy;
  const PC sCv = (PC)s.Cv, sD = (PC)s.D, sDv = (PC)s.Dv;
  const PD sP = (PD)s.P, sGM = (PD)s.GM, sY = (PD)s.Y, sK = (PD)s.K;
  const PF sGw = (PF)s.Gw, sGwU = NAFF == 2 ? (PF)s.Gw + 12 * N : nullptr;
  // ---- backward Riccati recursion on the f64 matrix cores.  Lane (c, g) = (lane & 15,
  // lane >> 4) holds, of a 12x12 matrix X padded to 16x16, the three entries X[4q + g][c]:
  // that is the B operand of X (pass q carries k = 4q + g), the A operand of X', and the
  // layout a product comes out in (row g + 4 reg, column c) -- so products chain from
  // register to register.  Column 12 of the B side carries the affine part (d, s, kappa, q),
  // column 13 the adjoint's (0, s', kappa', q').
  const int c = lane & 15, g = lane >> 4;
  const int cl = min(c, 11), cleg = cl / 3, cax = cl - 3 * cleg;
  const bool aff = c == 12 || (NAFF == 2 && c == 13);
  double adg[3];  // [Ad | gd | 0] in that layout; qreg: q_{k+1}, q'_{k+1} on lanes c == 12, 13
#pragma unroll
  for (int q_ = 0; q_ < 3; ++q_) {
    const int rq = 4 * q_ + g;
    adg[q_] = c < 12 ? (double)sAd[rq * 12 + c] : (c == 12 ? (double)sGX[rq] : 0.0);
    qreg[q_] = 0.0;
  }
  for (int k = N - 1; k >= 0; --k) {
    const float* const Bk = sBd + k * 144;
    const PC Dk = sD + k * 12;
    const PD Kk = sK + (keep_steps ? k : 0) * lq_slot(NAFF);
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
      // s, used on lanes c == 12; s' on lanes c == 13, with r = gw_u,k / 2 in that column
      if constexpr (NAFF == 2) {
        sreg[q_] = c == 13 ? fma(0.5, (double)sGw[k * 12 + rq], qreg[q_])
                           : qreg[q_] - sQ[rq] * (double)sXr[k * 12 + rq];
        rb[q_] = c == 13 ? 0.5 * (double)sGwU[k * 12 + rq] : 0.0;
      } else if constexpr (TAN) {
        sreg[q_] = qreg[q_] + s.Ts[k * 12 + rq];
        rb[q_] = c == 12 ? s.Tr[k * 12 + rq] : 0.0;
      } else {
        sreg[q_] = qreg[q_] - sQ[rq] * (double)sXr[k * 12 + rq];
      }
    }
    const gain_d4 zero = {0.0, 0.0, 0.0, 0.0};
    gain_d4 SW = gain_mm(sa, wv, zero);  // [S Ad | S d | 0]
    gain_d4 SB = gain_mm(sa, bt, zero);  // S Bt
    double swb[3], sbb[3];
#pragma unroll
    for (int r_ = 0; r_ < 3; ++r_) {
      swb[r_] = aff ? SW[r_] + sreg[r_] : SW[r_];  // columns 12, 13: S d + s, s'
      sbb[r_] = SB[r_];
    }
    gain_d4 G = gain_mm(bt, sbb, zero);  // Bt'S Bt
    gain_d4 M = gain_mm(bt, swb, zero);  // [Bt'S Ad | Bt'(S d + s) | Bt's']
    // [G | M] to LDS, G = Bt'S Bt + D with 1 on the diagonal of a slot not in use; column 13
    // of M takes Z'r on the slots in use
    if (c < 12 + NAFF) {
#pragma unroll
      for (int r_ = 0; r_ < 3; ++r_) {
        const int i = g + 4 * r_;
        if (c < 12) sGM[i * GW + c] = c == i ? G[r_] + (Dk[i] != 0.0 ? Dk[i] : 1.0) : G[r_];
        double m = M[r_];
        if constexpr (NAFF == 2) {
          if (c == 13 && Dk[i] != 0.0) {
            const int leg = i / 3, ax = i - 3 * leg;
            const PF ru = sGwU + k * 12 + 3 * leg;
            const double zr = ax == 2 ? fma((double)sZx[k * 4 + leg], (double)ru[0],
                                            fma((double)sZy[k * 4 + leg], (double)ru[1], (double)ru[2]))
                                      : (double)ru[ax];
            m = fma(0.5, zr, m);
          }
        }
        if constexpr (TAN) {  // column 12 of M takes Z'r on the slots in use
          if (c == 12 && Dk[i] != 0.0) {
            const int leg = i / 3, ax = i - 3 * leg;
            const double* const ru = s.Tr + k * 12 + 3 * leg;
            m += ax == 2 ? fma((double)sZx[k * 4 + leg], ru[0],
                               fma((double)sZy[k * 4 + leg], ru[1], ru[2]))
                         : ru[ax];
          }
        }
        sGM[i * GW + 12 + c] = m;
      }
    }
    __syncthreads();
    // eliminate, one column per lane (lanes past the last repeat it), then back-substitute the
    // 12 + NAFF right-hand sides on lanes 12 .., column by column: once y[j] is known every row
    // above takes its term, so the dependent chain is two operations per unknown
    {
      const int cc = min(lane, GW - 1);
      double col[12], rp[12], y[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) col[i] = sGM[i * GW + cc];
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
      if (lane >= 12 && lane < GW) {
#pragma unroll
        for (int i = 0; i < 12; ++i) sY[i * YW + lane - 12] = -y[i];
      }
    }
    __syncthreads();
    // [K_k | kappa_k | kappa'_k] = Z [Kp | kp | kp'] + [0 | c_k | 0] as a B operand; kept in LDS
    // for the forward pass and the outputs
    double kb[3], ka[3], kpb[3], kt[3];
    const int cy = min(c, YW - 1);
#pragma unroll
    for (int q_ = 0; q_ < 3; ++q_) {
      const int rq = 4 * q_ + g, leg = rq / 3, ax = rq - 3 * leg;
      const double yv = sY[rq * YW + cy];
      double v = yv;
      if (ax < 2)
        v = fma((double)(ax == 0 ? sZx[k * 4 + leg] : sZy[k * 4 + leg]),
                sY[(3 * leg + 2) * YW + cy], v);
      if (c == 12) v += sCv[k * 12 + rq];
      kb[q_] = c < YW ? v : 0.0;
      kpb[q_] = c < YW ? yv : 0.0;
      ka[q_] = c < 12 ? yv * Dk[rq] : 0.0;
      if constexpr (NAFF == 2 || TAN) kt[q_] = c < 12 ? v : 0.0;  // A operand K_k'
      if (c < 12) Kk[rq * 12 + c] = v;
      else if (c < YW) Kk[12 * c + rq] = v;  // kappa_k at 144, kappa'_k at 156
    }
    gain_d4 ad0 = {adg[0], adg[1], adg[2], 0.0};
    if constexpr (TAN) {  // e_k in gd's place
      if (c == 12) ad0 = {s.Te[k * 12 + g], s.Te[k * 12 + 4 + g], s.Te[k * 12 + 8 + g], 0.0};
    }
    // [A_cl | d_cl | d'_cl] = [Ad | gd | 0] + Bd_k [K_k | kappa_k | kappa'_k]
    gain_d4 AC = gain_mm(ab, kb, ad0);
    double acb[3], sacb[3];
#pragma unroll
    for (int r_ = 0; r_ < 3; ++r_) acb[r_] = AC[r_];
    gain_d4 SAC = gain_mm(sa, acb, zero);  // [S A_cl | S d_cl | S d'_cl]
#pragma unroll
    for (int r_ = 0; r_ < 3; ++r_) sacb[r_] = aff ? SAC[r_] + sreg[r_] : SAC[r_];
    gain_d4 Pn = gain_mm(acb, sacb, zero);  // [A_cl'S A_cl | A_cl'(S d_cl + s) | A_cl'(S d'_cl + s')]
    Pn = gain_mm(ka, kpb, Pn);              // + [Kp'D Kp | Kp'D kp | Kp'D kp']
    if constexpr (NAFF == 2 || TAN) Pn = gain_mm(kt, rb, Pn);  // + [0 | 0 | K_k'r] (TAN: column 12)
#pragma unroll
    for (int r_ = 0; r_ < 3; ++r_) {
      if (c < 12) sP[(g + 4 * r_) * 12 + c] = Pn[r_];
      qreg[r_] = Pn[r_];  // q_k, q'_k on lanes c == 12, 13
    }
    __syncthreads();
  }
}

// The trajectories of a forward pass: x_0 .. x_N [12 (N + 1)], u_0 .. u_{N-1} [12 N], and the
// adjoint's dx, du (ADJ)
struct GainTraj { double *X, *U, *DX, *DU; };

// The forward pass u_k = K_k x_k + kappa_k, x_{k+1} = Ad x_k + Bd_k u_k + gd from x_0 over the
// slots the recursion left, whole trajectories kept in LDS: on lanes 0..11, and with ADJ the
// adjoint's (kappa', no gd, dx_0 = 0) beside it on lanes 32..43.  The caller's barrier stands
// before the call (the last step's of gain_recursion); the last step's barrier ends it.
template <bool ADJ>
__device__ __forceinline__ void gain_rollout(const ProblemLds& sp, const double* sK,
                                             const GainTraj& t, int N, int lane) {
  const int half = ADJ ? lane >> 5 : 0, li = ADJ ? lane & 31 : lane;
  double* const tx = half ? t.DX : t.X;
  double* const tu = half ? t.DU : t.U;
  if (li < 12) tx[li] = half ? 0.0 : (double)sp.GX[12 + li];
  __syncthreads();
  for (int k = 0; k < N; ++k) {
    const double* const Kk = sK + k * lq_slot(ADJ ? 2 : 1);
    if (li < 12) {
      double acc = Kk[144 + 12 * half + li];
#pragma unroll
      for (int m = 0; m < 12; ++m) acc = fma(Kk[li * 12 + m], tx[k * 12 + m], acc);
      tu[k * 12 + li] = acc;
    }
    __syncthreads();
    if (li < 12) {
      double xn = half ? 0.0 : (double)sp.GX[li];
#pragma unroll
      for (int m = 0; m < 12; ++m) xn = fma((double)sp.Ad[li * 12 + m], tx[k * 12 + m], xn);
#pragma unroll
      for (int m = 0; m < 12; ++m) xn = fma((double)sp.Bd[(k * 12 + li) * 12 + m], tu[k * 12 + m], xn);
      tx[(k + 1) * 12 + li] = xn;
    }
    __syncthreads();
  }
}

}  // namespace cmpc
