// cmpc_problem.h -- what the evaluation kernels next to the solver (cmpc_kkt.hip, cmpc_gain.hip,
// cmpc_vjp.hip, cmpc_refine.hip) share: the problem part of their argument blocks, its image in LDS, the staging of an instance
// into it, the instance's constants with the validity decision, and the face rule.
// Included by cmpc_kkt.hip and, through cmpc_lq.h (what the last three share beyond this), by the
// other three only; the solve kernels have their own inputs and an fp32 face rule with a slack
// (cmpc_device.h, cmpc_polish.h faces_at).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cmpc.h"

namespace cmpc {

// the leading fields of KktArgs and of HeldArgs (cmpc_lq.h: GainArgs, VjpArgs, RefineArgs)
struct ProblemArgs {
  int N;
  float Q2[12], R2[12];  // the plan's constants: 2Q, 2R
  float mu, fz_min;
  double tol;            // face tolerance (face_rule)
  const float *Ad, *Bd, *gd, *x0, *xref;
  const uint8_t* contact;
  const float *mu_b, *fz_b, *Q, *R;  // nullable per-instance values
};

// the staged instance
struct __attribute__((aligned(16))) ProblemLds {
  float Bd[16 * 144];
  float Ad[144];
  float Xr[12 * 16];
  float GX[24];     // gd, x0
  double Q[12], R[12];
  uint8_t C[64];    // contact [4][N]
};

// what problem_issue has in flight: the loaded registers and the clamped indices
struct ProblemLoads {
  float4 vB[9], vA, vX, vG;
  uint8_t c;
  int eB[9], eA, eX, eG, eC, e12;
  float q2, r2, mu_l, fz_l, q_l, r_l;
};

// q, r: entry min(lane, 11) of the instance's Q, R; valid: the same decision in every lane
struct ProblemConsts { double mu, fz_min, q, r; bool valid; };

// Issue every load of instance b's problem; nothing is waited for.  A kernel issues its own loads
// right after this call (eX = min(lane, 3N - 1) and eC = min(lane, 4N - 1) index its 12N-float
// and 4N-byte arrays) and only then calls problem_commit, so that all of them are in flight
// together.
__device__ inline ProblemLoads problem_issue(const ProblemArgs& a, int64_t b, int lane) {
  ProblemLoads v;
  const int N = a.N;
  // the instance's constants (lanes past 11 repeat entry 11), selected into locals: with v's
  // fields written in the loop, the chain of selects is compiled as a tree of branches
  const int e12 = min(lane, 11);
  float q2 = 0.f, r2 = 0.f;
#pragma unroll
  for (int i = 0; i < 12; ++i)
    if (e12 == i) { q2 = a.Q2[i]; r2 = a.R2[i]; }
  v.e12 = e12, v.q2 = q2, v.r2 = r2;
  // (an absent array reads a word of gd instead, which is dropped: a load under a branch
  // would be waited for at the branch's end)
  const float* const dummy = a.gd + b * 12;
  v.mu_l = *(a.mu_b ? a.mu_b + b : dummy), v.fz_l = *(a.fz_b ? a.fz_b + b : dummy);
  v.q_l = (a.Q ? a.Q + b * 12 : dummy)[e12], v.r_l = (a.R ? a.R + b * 12 : dummy)[e12];
  // Load and LDS indices are clamped into the instance instead of predicated (lanes past the
  // end repeat its last element): a predicated copy is compiled as load-wait-store per
  // piece, which leaves one load in flight instead of all of them.
  const float4* gB = reinterpret_cast<const float4*>(a.Bd + b * N * 144);
#pragma unroll
  for (int t = 0; t < 9; ++t) v.vB[t] = gB[v.eB[t] = min(lane + 64 * t, 36 * N - 1)];
  v.eA = min(lane, 35), v.eX = min(lane, 3 * N - 1), v.eG = min(lane, 5);
  v.eC = min(lane, 4 * N - 1);
  v.vA = reinterpret_cast<const float4*>(a.Ad + b * 144)[v.eA];
  v.vX = reinterpret_cast<const float4*>(a.xref + b * N * 12)[v.eX];
  v.vG = v.eG < 3 ? reinterpret_cast<const float4*>(a.gd + b * 12)[v.eG]
                  : reinterpret_cast<const float4*>(a.x0 + b * 12)[v.eG - 3];
  v.c = a.contact[b * N * 4 + v.eC];
  return v;
}

// the first wait: the loads of problem_issue to LDS
__device__ inline void problem_commit(ProblemLds& s, const ProblemLoads& v) {
#pragma unroll
  for (int t = 0; t < 9; ++t) reinterpret_cast<float4*>(s.Bd)[v.eB[t]] = v.vB[t];
  reinterpret_cast<float4*>(s.Ad)[v.eA] = v.vA;
  reinterpret_cast<float4*>(s.Xr)[v.eX] = v.vX;
  reinterpret_cast<float4*>(s.GX)[v.eG] = v.vG;
  s.C[v.eC] = v.c;
}

// The instance's mu, fz_min, Q, R (a per-instance value or the plan's), Q and R to LDS, and
// whether the entries are valid (the rules of cmpc_solve_io_run).  The caller's barrier follows.
__device__ inline ProblemConsts problem_consts(const ProblemArgs& a, ProblemLds& s,
                                               const ProblemLoads& v) {
  ProblemConsts k;
  k.mu = (double)(a.mu_b ? v.mu_l : a.mu), k.fz_min = (double)(a.fz_b ? v.fz_l : a.fz_min);
  k.q = a.Q ? (double)v.q_l : 0.5 * (double)v.q2, k.r = a.R ? (double)v.r_l : 0.5 * (double)v.r2;
  s.Q[v.e12] = k.q;
  s.R[v.e12] = k.r;
  k.valid = !__any(!(k.q >= 0.0 && isfinite(k.q) && k.r > 0.0 && isfinite(k.r))) &&
            k.mu > 0.0 && isfinite(k.mu) && isfinite(k.fz_min);
  return k;
}

// The faces a stance force holds, as CMPC_FACE_* bits (cmpc/duals.py recover): within
// tol * max(1, |fz|) of the face, the + face of an axis tested before the - face.  Each product is
// rounded on its own, as NumPy does, so that a force on a threshold is classified the same way
// on both sides.
__device__ inline unsigned face_rule(double fx, double fy, double fz, double mu, double fz_min,
                                     double tol) {
#pragma clang fp contract(off)
  const double scale = tol * fmax(1.0, fabs(fz));
  const double mf = mu * fz;
  unsigned m = 0;
  if (fabs(fx - mf) <= scale) m |= CMPC_FACE_FX_POS;
  else if (fabs(fx + mf) <= scale) m |= CMPC_FACE_FX_NEG;
  if (fabs(fy - mf) <= scale) m |= CMPC_FACE_FY_POS;
  else if (fabs(fy + mf) <= scale) m |= CMPC_FACE_FY_NEG;
  if (fabs(fz - fz_min) <= scale) m |= CMPC_FACE_FZ_MIN;
  return m;
}

}  // namespace cmpc
