// cmpc_kkt.hip -- cost and KKT residuals of a batch of points of the reference QP, on the device
// (cmpc_kkt_run, include/cmpc.h).
//
// For each instance: cost = 1/2 w'Hw + g'w and the three residuals oracle/mpc_qp.kkt_residuals
// defines for the QP oracle/mpc_qp.build_qp assembles (CasADi's convention):
//   stat = max |H w + g + A' lam_a + lam_x|
//   prim = the largest violation of lba <= A w <= uba, lbx <= w <= ubx
//   comp = max over the multipliers of  max(lam, 0) |ub - v|,  max(-lam, 0) |v - lb|,
//          +inf where a multiplier has the sign of an infinite bound
// H, A and the bounds are never formed: the rows are
//   dynamics (k, i)    x_{k+1}[i] - Ad[i] x_k - Bd_k[i] u_k = gd[i] (+ Ad[i] x_0 for k = 0)
//   friction (k, l, r) +-f - mu fz <= 0 on a stance leg, free on a swing leg
//   bounds             fz >= fz_min on a stance leg, f = 0 on a swing leg, states free.
// With lam == NULL the multipliers are first recovered from w by the rule of cmpc/duals.py
// (backward adjoint, then the faces the forces hold).
//
// One 64-lane wave per instance, everything in fp64 on the fp32 inputs widened exactly.  The
// wave stages the instance in LDS with coalesced 16-byte loads (all issued before the first is
// used: ~15 KB in flight per wave; the problem's part by cmpc_problem.h, shared with
// cmpc_gain.hip), the multipliers as doubles; then every (step, row) is one
// lane's sequential sum in a fixed order, and the four results are butterfly reductions over the
// lanes: bitwise repeatable, independent of B and of the instance's place in the batch.  The
// adjoint recursion is the only serial part (N steps of a 12-term product on 12 lanes).
// No atomics, no workspace.
//
// This file is compiled as part of cmpc_host.hip (single translation unit).
#include "cmpc_problem.h"

namespace cmpc {

struct KktArgs {
  ProblemArgs p;
  const float* w;
  const float* lam;      // nullable: recovered with p.tol
  double* res;
};

// max that keeps a NaN once it has seen one (np.max)
__device__ inline double kkt_max(double m, double a) { return (a > m || a != a) ? a : m; }

__device__ inline double kkt_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = kkt_max(v, __shfl_xor(v, o));
  return v;
}

__device__ inline double kkt_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// one multiplier's complementarity term (kkt_residuals' comp): lo / hi may be infinite
__device__ inline double kkt_comp(double lam, double v, double lo, double hi) {
  if (lam > 0.0) return isfinite(hi) ? lam * fabs(hi - v) : INFINITY;
  if (lam < 0.0) return isfinite(lo) ? -lam * fabs(v - lo) : INFINITY;
  return lam != lam ? lam : 0.0;
}

// The multipliers of one (step, leg) from s = 2R u - Bd' lam_eq restricted to the leg
// (cmpc/duals.py recover): the faces it holds by face_rule, a multiplier per held face.  rz too
// rounds its product on its own, as NumPy does.
__device__ inline void kkt_recover_leg(bool stance, const double s[3], double fx, double fy,
                                       double fz, double mu, double fz_min, double tol,
                                       double lf[4], double lx[3]) {
#pragma clang fp contract(off)
  lf[0] = lf[1] = lf[2] = lf[3] = 0.0;
  lx[0] = lx[1] = lx[2] = 0.0;
  if (!stance) {
    lx[0] = -s[0];
    lx[1] = -s[1];
    lx[2] = -s[2];
    return;
  }
  const unsigned m = face_rule(fx, fy, fz, mu, fz_min, tol);
  if (m & CMPC_FACE_FX_POS) lf[0] = fmax(-s[0], 0.0);
  if (m & CMPC_FACE_FX_NEG) lf[1] = fmax(s[0], 0.0);
  if (m & CMPC_FACE_FY_POS) lf[2] = fmax(-s[1], 0.0);
  if (m & CMPC_FACE_FY_NEG) lf[3] = fmax(s[1], 0.0);
  const double rz = s[2] - mu * (((lf[0] + lf[1]) + lf[2]) + lf[3]);  // = -lam_x[fz]
  if (m & CMPC_FACE_FZ_MIN) lx[2] = fmin(-rz, 0.0);  // active lower bound: lam <= 0
}

__global__ void __launch_bounds__(64) kkt_kernel(KktArgs a, int64_t B) {
  __shared__ ProblemLds sp;
  __shared__ __attribute__((aligned(16))) float sW[24 * 16];   // [x_1..x_N | u_0..u_{N-1}]
  __shared__ __attribute__((aligned(16))) double sL[52 * 16];  // [lam_x | lam_a], lam's layout
  auto& [sBd, sAd, sXr, sGX, sQ, sR, sC] = sp;
  const int lane = threadIdx.x;
  const int N = a.p.N;
  double* const Lx = sL;            // lam_x: states [0, 12N), forces [12N, 24N)
  double* const Ld = sL + 24 * N;   // lam_a, dynamics rows
  double* const Lf = sL + 36 * N;   // lam_a, friction rows [(k, leg)][4]
  const float* const sU = sW + 12 * N;

  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    // ---- stage the instance: the problem's loads, then w's and lam's, all issued before the
    // first LDS write waits for one (indices clamped, not predicated: problem_issue)
    const ProblemLoads ld = problem_issue(a.p, b, lane);
    {
      const float4* gW = reinterpret_cast<const float4*>(a.w + b * N * 24);
      const float4* gL = a.lam ? reinterpret_cast<const float4*>(a.lam + b * N * 52) : nullptr;
      float4 vW[2], vL[4];
      int eW[2], eL[4];
#pragma unroll
      for (int t = 0; t < 2; ++t) vW[t] = gW[eW[t] = min(lane + 64 * t, 6 * N - 1)];
      if (gL) {
#pragma unroll
        for (int t = 0; t < 4; ++t) vL[t] = gL[eL[t] = min(lane + 64 * t, 13 * N - 1)];
      }
      problem_commit(sp, ld);
#pragma unroll
      for (int t = 0; t < 2; ++t) reinterpret_cast<float4*>(sW)[eW[t]] = vW[t];
      if (gL) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          reinterpret_cast<double2*>(sL)[2 * eL[t]] = make_double2((double)vL[t].x, (double)vL[t].y);
          reinterpret_cast<double2*>(sL)[2 * eL[t] + 1] = make_double2((double)vL[t].z, (double)vL[t].w);
        }
      }
    }
    const ProblemConsts pc = problem_consts(a.p, sp, ld);
    const double mu = pc.mu, fz_min = pc.fz_min, q = pc.q;
    __syncthreads();
    // an invalid entry gives four NaNs; the same decision in every lane
    if (!pc.valid) {
      if (lane < 4) a.res[b * 4 + lane] = __builtin_nan("");
      __syncthreads();
      continue;
    }

    // ---- lam == NULL: recover the multipliers (cmpc/duals.py recover)
    if (!a.lam) {
      for (int e = lane; e < 12 * N; e += 64) Lx[e] = 0.0;  // states carry no bound multiplier
      // backward adjoint on lanes 0..11: nu_k = Ad' nu_{k+1} - 2Q (x_{k+1} - xref_k), nu_N = 0
      double adc[12];  // column `lane` of Ad
#pragma unroll
      for (int i = 0; i < 12; ++i) adc[i] = lane < 12 ? (double)sAd[i * 12 + lane] : 0.0;
      for (int k = N - 1; k >= 0; --k) {
        if (lane < 12) {
          double acc = 0.0;
          if (k < N - 1) {
#pragma unroll
            for (int i = 0; i < 12; ++i) acc = fma(adc[i], Ld[(k + 1) * 12 + i], acc);
          }
          Ld[k * 12 + lane] =
              acc - 2.0 * q * ((double)sW[k * 12 + lane] - (double)sXr[k * 12 + lane]);
        }
        __syncthreads();
      }
      // one lane per (step, leg): s = 2R u - Bd_k' lam_eq[k] on the leg, then its faces
      if (lane < 4 * N) {
        const int k = lane >> 2, leg = lane & 3;
        double s[3], f[3], lf[4], lx[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int j = 3 * leg + c;
          f[c] = (double)sU[k * 12 + j];
          double acc = 2.0 * sR[j] * f[c];
#pragma unroll
          for (int i = 0; i < 12; ++i)
            acc = fma(-(double)sBd[(k * 12 + i) * 12 + j], Ld[k * 12 + i], acc);
          s[c] = acc;
        }
        kkt_recover_leg(sC[leg * N + k] != 0, s, f[0], f[1], f[2], mu, fz_min, a.p.tol, lf, lx);
#pragma unroll
        for (int c = 0; c < 3; ++c) Lx[12 * N + k * 12 + 3 * leg + c] = lx[c];
#pragma unroll
        for (int c = 0; c < 4; ++c) Lf[lane * 4 + c] = lf[c];
      }
      __syncthreads();
    }

    // ---- the residuals: one lane per (step, row), each a sequential sum in a fixed order
    double cost = 0.0, stat = 0.0, prim = 0.0, comp = 0.0;
    for (int row = lane; row < 12 * N; row += 64) {
      const int k = row / 12, i = row - 12 * k;
      const double qi = sQ[i], ri = sR[i];
      const double x = (double)sW[row], xr = (double)sXr[row], u = (double)sU[row];
      // dynamics row (k, i): A w - beq
      double aw = x;
      if (k > 0) {
#pragma unroll
        for (int j = 0; j < 12; ++j)
          aw = fma(-(double)sAd[i * 12 + j], (double)sW[(k - 1) * 12 + j], aw);
      }
#pragma unroll
      for (int j = 0; j < 12; ++j)
        aw = fma(-(double)sBd[row * 12 + j], (double)sU[k * 12 + j], aw);
      double beq = (double)sGX[i];
      if (k == 0) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 12; ++j) acc = fma((double)sAd[i * 12 + j], (double)sGX[12 + j], acc);
        beq = acc + beq;
      }
      const double ld = Ld[row];
      prim = kkt_max(prim, fabs(aw - beq));
      comp = kkt_max(comp, kkt_comp(ld, aw, beq, beq));
      // stationarity in x_{k+1}[i]: 2Q (x - xref) + lam_eq[k] - Ad' lam_eq[k+1] + lam_x
      const double lxs = Lx[row];
      double st = 2.0 * qi * x - 2.0 * qi * xr + ld;
      if (k + 1 < N) {
#pragma unroll
        for (int m = 0; m < 12; ++m) st = fma(-(double)sAd[m * 12 + i], Ld[(k + 1) * 12 + m], st);
      }
      st += lxs;
      stat = kkt_max(stat, fabs(st));
      comp = kkt_max(comp, kkt_comp(lxs, x, -INFINITY, INFINITY));
      cost += qi * x * x - 2.0 * qi * xr * x;
      // stationarity in u_k[i]: 2R u - Bd_k' lam_eq[k] + F' lam_fric + lam_x
      const int leg = i / 3, ax = i - 3 * leg;
      const bool stance = sC[leg * N + k] != 0;
      const double* lf = Lf + (k * 4 + leg) * 4;
      const double lxu = Lx[12 * N + row];
      double su = 2.0 * ri * u;
#pragma unroll
      for (int m = 0; m < 12; ++m) su = fma(-(double)sBd[(k * 12 + m) * 12 + i], Ld[k * 12 + m], su);
      if (ax == 0) su += lf[0] - lf[1];
      else if (ax == 1) su += lf[2] - lf[3];
      else su += -mu * lf[0] - mu * lf[1] - mu * lf[2] - mu * lf[3];
      su += lxu;
      stat = kkt_max(stat, fabs(su));
      // bounds on u_k[i]: swing 0 <= u <= 0, stance fz >= fz_min, fx / fy free
      if (!stance) {
        prim = kkt_max(prim, fabs(u));
        comp = kkt_max(comp, kkt_comp(lxu, u, 0.0, 0.0));
      } else if (ax == 2) {
        prim = kkt_max(prim, kkt_max(0.0, fz_min - u));
        comp = kkt_max(comp, kkt_comp(lxu, u, fz_min, INFINITY));
      } else {
        comp = kkt_max(comp, kkt_comp(lxu, u, -INFINITY, INFINITY));
      }
      cost += ri * u * u;
    }
    // friction rows of one (step, leg) per lane: +-fx - mu fz, +-fy - mu fz (<= 0 in stance)
    if (lane < 4 * N) {
      const int k = lane >> 2, leg = lane & 3;
      const bool stance = sC[leg * N + k] != 0;
      const double fx = (double)sU[k * 12 + 3 * leg], fy = (double)sU[k * 12 + 3 * leg + 1],
                   fz = (double)sU[k * 12 + 3 * leg + 2];
      const double hi = stance ? 0.0 : INFINITY;
      const double rows[4] = {fx - mu * fz, -fx - mu * fz, fy - mu * fz, -fy - mu * fz};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (stance) prim = kkt_max(prim, kkt_max(0.0, rows[c]));
        comp = kkt_max(comp, kkt_comp(Lf[lane * 4 + c], rows[c], -INFINITY, hi));
      }
    }
    cost = kkt_wave_sum(cost);
    stat = kkt_wave_max(stat);
    prim = kkt_wave_max(prim);
    comp = kkt_wave_max(comp);
    const double out = lane == 0 ? cost : (lane == 1 ? stat : (lane == 2 ? prim : comp));
    if (lane < 4) a.res[b * 4 + lane] = out;
    __syncthreads();  // the next instance overwrites the staged arrays
  }
}

}  // namespace cmpc
