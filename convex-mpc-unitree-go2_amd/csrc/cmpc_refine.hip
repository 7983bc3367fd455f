// cmpc_refine.hip -- certified float64 refinement of a batch of solved instances: a primal-dual
// active-set loop around the optimum on the held faces, which replaces an answer only when the
// float64 KKT conditions hold on the whole QP (cmpc_refine_run, include/cmpc.h).
//
// Per instance the masks of the held faces are read from `faces` or off w's forces (face_rule),
// as gain_kernel does.  Then, round r = 0, 1, ..:
//   1. (u, x): the optimum on the held faces and its rollout -- gain_recursion<1> and
//      gain_rollout<false>
//   2. costate  p_k = 2Q (x_{k+1} - xref_k) + Ad' p_{k+1},  p_N = 0;   g_k = 2R u_k + Bd_k' p_k
//   3. per stance leg, (gx, gy, gz) its part of g_k: a held sx mu face of x has
//      lam_x = -sx gx (the same for y), a face not held 0, a held fz face
//      lam_z = gz - mu (lam_x + lam_y)
//   4. us = max(1, max|u|), gs = us min_i 2R_i.  Violated: a face not held whose row
//      fx - mu fz, -fx - mu fz, fy - mu fz, -fy - mu fz, fz_min - fz is above prim_tol us (of two
//      violated signs of an axis only the larger row counts, the + face on a tie).  Negative: a
//      held face with lam < -dual_tol gs.
//   5. neither: certified after r repairs.  r == max_rounds: ROUNDS.  Any face violated: every
//      violated face is added (the other sign of its axis cleared), nothing dropped; else every
//      negative face is dropped.  The new masks equal those of an earlier round: CYCLE.
// One lane per (step, leg) holds the mask, tests the faces and forms the multipliers; every
// decision is a ballot, so each branch on one is wave-uniform.  The masks of the rounds so far
// stay in LDS (64 bytes a round) for the cycle test.  Every round restarts the recursion at step
// N - 1 (the restart at the highest changed step is not built).
//
// One 64-lane wave per instance, fp64 on the fp32 inputs widened exactly, staged by
// cmpc_problem.h.  Every sum runs in an order the code fixes (the maxima are order-free):
// bitwise repeatable, independent of B and of the instance's place in the batch.  Plain stores,
// no atomics, no workspace.  w_out may be w: an instance's forces are staged before its row is
// written, by the same wave.
//
// This file is compiled as part of cmpc_host.hip (single translation unit).  The staging of the
// held faces, the mask and its affine set, the recursion and the forward pass are cmpc_lq.h's, as
// they are in cmpc_gain.hip and cmpc_vjp.hip.
#include "cmpc_lq.h"

namespace cmpc {

struct RefineArgs : HeldArgs {  // w: the input answer too (its forces' faces when faces == NULL)
  int max_rounds;
  double prim_tol, dual_tol;
  int32_t* info;
  double *res, *w64, *lam;  // nullable
  uint8_t* faces_out;       // nullable
  float* w_out;             // nullable, may alias w
  int32_t* status;          // nullable
};

constexpr int kRefineRounds = 17;  // rounds 0 .. CMPC_REFINE_MAX_ROUNDS

// max / min of v over the wave (order-free)
__device__ inline double refine_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// The rows of a stance leg's faces at the force f, in the mask's bit order (fz_min - fz,
// fx - mu fz, -fx - mu fz, fy - mu fz, -fy - mu fz).  Each product is rounded on its own, as
// NumPy does.
__device__ inline void refine_rows(double fx, double fy, double fz, double mu, double fz_min,
                                   double v[5]) {
#pragma clang fp contract(off)
  const double mf = mu * fz;
  v[0] = fz_min - fz;
  v[1] = fx - mf;
  v[2] = -fx - mf;
  v[3] = fy - mf;
  v[4] = -fy - mf;
}

__global__ void __launch_bounds__(64) refine_kernel(RefineArgs a, int64_t B) {
  __shared__ ProblemLds sp;
  auto& [sBd, sAd, sXr, sGX, sQ, sR, sC] = sp;
  __shared__ float sZx[64], sZy[64];                           // per (step, leg): +-mu or 0, exact
  __shared__ double sCv[12 * 16], sD[12 * 16];                 // c_k and diag(Z'RZ) per step
  __shared__ double sDv[12 * 16];                              // d_k = Bd_k c_k + gd per step
  __shared__ double sP[144];                                   // P_k as computed
  __shared__ __attribute__((aligned(16))) double sGM[12 * 25];  // [G | rhs]
  __shared__ double sY[12 * 13];                               // [Kp | kp]
  __shared__ __attribute__((aligned(16))) float sUin[12 * 16];  // w's forces (xref where w is absent)
  __shared__ uint8_t sHist[kRefineRounds][64];                 // the masks of every round so far
  __shared__ double sX[12 * 17], sUu[12 * 16];                 // x_0 .. x_N, u_0 .. u_{N-1}
  __shared__ double sCo[12 * 17], sG[12 * 16];                 // p_0 .. p_N, g_0 .. g_{N-1}
  extern __shared__ double sK[];  // N slots of (K_k [12][12], kappa_k [12])
  const int lane = threadIdx.x;
  const int N = a.p.N;
  const double nan = __builtin_nan("");
  const GainLds s{sZx, sZy, sCv, sD, sDv, sP, sGM, sY, sK};

  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    // ---- stage the instance as gain_kernel does: the problem's loads, the given faces and the
    // forces of w (held_issue), all issued before the first LDS write waits for one
    const ProblemLoads ld = problem_issue(a.p, b, lane);
    const HeldLoads hl = held_issue(a, ld, b);
    problem_commit(sp, ld);
    reinterpret_cast<float4*>(sUin)[ld.eX] = hl.vU;
    const ProblemConsts pc = problem_consts(a.p, sp, ld);
    const double mu = pc.mu, fz_min = pc.fz_min;
    __syncthreads();

    // ---- one lane per (step, leg): the mask.  A given mask with both signs of an axis (an
    // apex, and every inconsistent mask is one) is not refined; face_rule never gives one.
    const int k_ = lane >> 2, leg_ = lane & 3;
    const bool stance = lane < 4 * N && sC[leg_ * N + k_] != 0;
    unsigned mask = 0;
    if (stance) mask = held_mask(a, hl, sUin, lane, pc);
    const bool apex = (mask & 6u) == 6u || (mask & 24u) == 24u;
    // an apex mask or an invalid entry: NaN in the fp64 outputs, 0xFF in faces_out, w_out and
    // status untouched; the same decision in every lane
    if (__any(apex) || !pc.valid) {
      if (lane == 0) a.info[b] = CMPC_REFINE_INVALID;
      if (a.res && lane < 3) a.res[b * 3 + lane] = nan;
      if (a.w64)
        for (int e = lane; e < 24 * N; e += 64) a.w64[b * 24 * N + e] = nan;
      if (a.lam)
        for (int e = lane; e < 52 * N; e += 64) a.lam[b * 52 * N + e] = nan;
      if (a.faces_out && lane < 4 * N) a.faces_out[b * 4 * N + lane] = 0xFF;
      __syncthreads();
      continue;
    }
    double r2min = 2.0 * sR[0];  // min_i 2R_i
#pragma unroll
    for (int i = 1; i < 12; ++i) r2min = fmin(r2min, 2.0 * sR[i]);

    // ---- the rounds
    int info;
    double lamf[4], lamz, vmax, lmin, us, gs;  // of the last round
    for (int r = 0;; ++r) {
      // the affine set of the lane's mask (its verdict is the apex test above) and the affine
      // terms, then 1. the optimum on the held faces and its rollout
      sHist[r][lane] = (uint8_t)mask;
      if (lane < 4 * N) gain_leg_fill(sp, s, lane, mask, stance, pc);
      gain_affine(sp, s, N, lane);
      double qreg[3];  // (q_0: not used)
      gain_recursion<1>(sp, s, N, 1, lane, qreg);
      gain_rollout<false>(sp, sK, GainTraj{sX, sUu, nullptr, nullptr}, N, lane);

      // 2. the costate pass, then g_k of every step
      if (lane < 12) sCo[N * 12 + lane] = 0.0;
      __syncthreads();
      for (int k = N - 1; k >= 0; --k) {
        if (lane < 12) {
          double acc = 2.0 * sQ[lane] * (sX[(k + 1) * 12 + lane] - (double)sXr[k * 12 + lane]);
#pragma unroll
          for (int m = 0; m < 12; ++m) acc = fma((double)sAd[m * 12 + lane], sCo[(k + 1) * 12 + m], acc);
          sCo[k * 12 + lane] = acc;
        }
        __syncthreads();
      }
      for (int e = lane; e < 12 * N; e += 64) {
        const int k = e / 12, j = e - 12 * k;
        double acc = 2.0 * sR[j] * sUu[e];
#pragma unroll
        for (int i = 0; i < 12; ++i) acc = fma((double)sBd[(k * 12 + i) * 12 + j], sCo[k * 12 + i], acc);
        sG[e] = acc;
      }
      __syncthreads();

      // 3., 4. the lane's multipliers and face tests
      double f[3] = {0.0, 0.0, 0.0}, v[5];
      lamf[0] = lamf[1] = lamf[2] = lamf[3] = lamz = 0.0;
      if (stance) {
        const double* const gk = sG + k_ * 12 + 3 * leg_;
#pragma unroll
        for (int x = 0; x < 3; ++x) f[x] = sUu[k_ * 12 + 3 * leg_ + x];
        if (mask & 2u) lamf[0] = -gk[0];
        if (mask & 4u) lamf[1] = gk[0];
        if (mask & 8u) lamf[2] = -gk[1];
        if (mask & 16u) lamf[3] = gk[1];
        if (mask & 1u) lamz = gk[2] - mu * (((lamf[0] + lamf[1]) + lamf[2]) + lamf[3]);
      }
      us = fmax(1.0, refine_wave_max(fmax(fabs(f[0]), fmax(fabs(f[1]), fabs(f[2])))));
      gs = us * r2min;
      unsigned vb = 0, nb = 0;
      double vl = 0.0, ll = 0.0;  // the lane's largest row of a face not held, its lowest multiplier
      if (stance) {
        refine_rows(f[0], f[1], f[2], mu, fz_min, v);
        const double pt = a.prim_tol * us, dt = -a.dual_tol * gs;
#pragma unroll
        for (int i = 0; i < 5; ++i)
          if (!(mask >> i & 1u)) {
            vl = fmax(vl, v[i]);
            if (v[i] > pt) vb |= 1u << i;
          }
        if ((vb & 6u) == 6u) vb &= v[1] >= v[2] ? ~4u : ~2u;
        if ((vb & 24u) == 24u) vb &= v[3] >= v[4] ? ~16u : ~8u;
        const double lm[5] = {lamz, lamf[0], lamf[1], lamf[2], lamf[3]};
#pragma unroll
        for (int i = 0; i < 5; ++i)
          if (mask >> i & 1u) {
            ll = fmin(ll, lm[i]);
            if (lm[i] < dt) nb |= 1u << i;
          }
      }
      vmax = refine_wave_max(vl);
      lmin = -refine_wave_max(-ll);

      // 5. decide: every condition is the same in every lane
      const bool anyv = __any(vb != 0), anyn = __any(nb != 0);
      if (!anyv && !anyn) { info = r; break; }
      if (r == a.max_rounds) { info = CMPC_REFINE_ROUNDS; break; }
      unsigned next = mask;
      if (anyv) {
        next |= vb;
        if (vb & 2u) next &= ~4u;
        if (vb & 4u) next &= ~2u;
        if (vb & 8u) next &= ~16u;
        if (vb & 16u) next &= ~8u;
      } else {
        next &= ~nb;
      }
      bool seen = false;
      for (int j = 0; j <= r; ++j) seen = seen || __all(sHist[j][lane] == (uint8_t)next);
      if (seen) { info = CMPC_REFINE_CYCLE; break; }
      mask = next;
    }

    // ---- outputs: the last round's point
    const bool cert = info >= 0;
    if (lane == 0) {
      a.info[b] = info;
      if (a.status && cert) a.status[b] = 1;
    }
    if (a.res) {
      double du = 0.0, um = 0.0;
      for (int e = lane; e < 12 * N; e += 64) {
        du = fmax(du, fabs(sUu[e] - (double)sUin[e]));
        um = fmax(um, fabs((double)sUin[e]));
      }
      du = refine_wave_max(du);
      um = refine_wave_max(um);
      if (lane == 0) {
        a.res[b * 3] = vmax / us;
        a.res[b * 3 + 1] = lmin / gs;
        a.res[b * 3 + 2] = a.w ? du / fmax(1.0, um) : nan;
      }
    }
    if (a.w64 || (a.w_out && cert))
      for (int e = lane; e < 24 * N; e += 64) {
        const double val = e < 12 * N ? sX[12 + e] : sUu[e - 12 * N];
        if (a.w64) a.w64[b * 24 * N + e] = val;
        if (a.w_out && cert) a.w_out[b * 24 * N + e] = (float)val;
      }
    if (a.lam) {  // [lam_x (24N) | lam_eq (12N) | lam_fric (N, 4, 4)], cmpc/duals.py recover
      double* const L = a.lam + b * 52 * N;
      for (int e = lane; e < 12 * N; e += 64) {
        L[e] = 0.0;
        L[24 * N + e] = -sCo[e];
      }
      if (lane < 4 * N) {
        double* const lx = L + 12 * N + 3 * lane;
        const double* const gk = sG + 3 * lane;
        lx[0] = stance ? 0.0 : -gk[0];
        lx[1] = stance ? 0.0 : -gk[1];
        lx[2] = stance ? -lamz : -gk[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) L[36 * N + 4 * lane + i] = lamf[i];
      }
    }
    if (a.faces_out && lane < 4 * N) a.faces_out[b * 4 * N + lane] = (uint8_t)mask;
    __syncthreads();  // the next instance overwrites the staged arrays
  }
}

}  // namespace cmpc
