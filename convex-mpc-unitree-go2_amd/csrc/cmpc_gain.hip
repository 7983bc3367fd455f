// cmpc_gain.hip -- feedback gain K = d u_0 / d x_0, value-function gradient and Hessian and the
// optimum on the held faces of a batch of solved instances (cmpc_gain_run, include/cmpc.h;
// DESIGN.md 4l).
//
// The LQ problem on the held faces, its backward recursion (K_k, kappa_k, P_k, q_k) and the
// helpers that evaluate it are cmpc_lq.h's, shared with cmpc_vjp.hip and cmpc_refine.hip; this
// kernel runs the recursion once and gives K = K_0, Vxx = 2 P_0, Vx = 2 (P_0 x_0 + q_0) and the
// forward pass u_k = K_k x_k + kappa_k.
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
#include "cmpc_lq.h"

namespace cmpc {

struct GainArgs : HeldArgs {
  double *K, *Vx, *Vxx, *u_star;  // all but K nullable
  uint8_t* faces_out;             // nullable
};

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
  const GainLds s{sZx, sZy, sCv, sD, sDv, sP, sGM, sY, sK};

  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    // ---- stage the instance: the problem's loads, then the given faces and the forces
    // (held_issue), all issued before the first LDS write waits for one
    const ProblemLoads ld = problem_issue(a.p, b, lane);
    const HeldLoads hl = held_issue(a, ld, b);
    problem_commit(sp, ld);
    reinterpret_cast<float4*>(sU)[ld.eX] = hl.vU;
    const ProblemConsts pc = problem_consts(a.p, sp, ld);
    __syncthreads();

    // ---- one lane per (step, leg): the mask, then its affine set
    bool ok = true;
    unsigned mask = 0;
    if (lane < 4 * N) {
      const bool stance = sC[(lane & 3) * N + (lane >> 2)] != 0;
      if (stance) mask = held_mask(a, hl, sU, lane, pc);
      ok = gain_leg_fill(sp, s, lane, mask, stance, pc);
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

    // ---- the affine terms, then the backward Riccati recursion on the f64 matrix cores
    gain_affine(sp, s, N, lane);
    const int c = lane & 15, g = lane >> 4;
    double qreg[3];
    gain_recursion<1>(sp, s, N, keep_steps, lane, qreg);
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
    // The forward pass streams u_k to global memory and keeps a single x in the buffers it shares
    // with the recursion, unlike gain_rollout: LDS for whole trajectories would cost a wave per
    // CU.
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
