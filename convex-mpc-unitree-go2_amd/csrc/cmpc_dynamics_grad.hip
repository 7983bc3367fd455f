// cmpc_dynamics_grad.hip -- reverse- and forward-mode derivatives of cmpc_dynamics.hip's closed
// form (cmpc_dynamics_vjp_run / cmpc_dynamics_jvp_run, include/cmpc.h), for a batch of robots.
//
// The function differentiated is what dynamics_kernel evaluates before it rounds, in fp64 on the
// fp32 inputs widened exactly.  With minv = 1/m, J = inertia^-1, Rt = R_z(yaw_avg)', and per
// (step k, leg l)  S = [r_kl]x,  W = J S,  V = Rt W,  the blocks of Bd_k[:, 3l:3l+3] are
//   rows 0-2 h2 minv I3,  rows 3-5 h2 V,  rows 6-8 dt minv I3,  rows 9-11 dt W     (h2 = dt^2/2)
// and Ad[3:6, 9:12] = dt Rt; everything else is constant.  Ac^2 = 0 makes this a polynomial in
// minv, J, S and Rt, so both derivatives are a handful of 3x3 products per (step, leg).
//
// Both kernels keep dynamics_kernel's shape: one 64-lane wave per robot, grid-stride over the
// batch, the per-robot scalars (1/m, I^-1 by the same adjugate, yaw_avg by the same LDS sum, so
// they are the primal's bit for bit) computed redundantly per lane from uniform loads, and
// lane = 4k + l owning one (step, leg).  Lanes at or past 4N contribute exact zeros.
//
// vjp_dynamics_kernel is HBM-bound on g_Bd (8 x 144 x N bytes per robot, 18 KB at N = 16): the
// wave moves it into LDS with 16-byte loads per lane, coalesced over the robot's contiguous
// N x 144 doubles, and each lane then reads its 12 x 3 block from LDS.  A step's rows are
// kDynGradStride = 154 doubles apart there (308 dwords = 20 mod 64), which spreads the 32 lanes of
// a ds_read_b64 group over the banks (at most 2-way on 8 of them; 144 would be 4-way on all).
// Only the 3-row groups that a wanted output reads are moved: G0 and G2 for g_mass, G1 and G3 for
// g_inertia and g_r_feet, G1 for g_yaw; a NULL g_Bd is never read.  The 14 sums over (k, l)
// (g_minv, the 9 entries of g_J, the 4 of g_Rt[0:2, 0:2]) each run through one xor-butterfly of
// six shuffle steps (32, 16, 8, 4, 2, 1): a fixed tree, the same value in every lane, no atomics.
//
// jvp_dynamics_kernel is the primal with tangents: d_Bd is staged in LDS as fp32 and stored with
// coalesced 16-byte stores, d_Ad is written whole.
//
// This file is compiled as part of cmpc_host.hip (single translation unit).
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cmpc {

constexpr int kDynGradStride = 154;  // doubles between the steps of the staged g_Bd

struct DynVjpArgs {
  const float *mass, *inertia, *r_feet, *xref;
  const double *g_Ad, *g_Bd;
  double *g_mass, *g_inertia, *g_r_feet, *g_yaw;
};

struct DynJvpArgs {
  const float *mass, *inertia, *r_feet, *xref;
  const float *d_mass, *d_inertia, *d_r_feet, *d_xref;
  float *d_Ad, *d_Bd;
};

// I^-1 = adjugate / det (row-major): dynamics_kernel's expressions, term for term
__device__ inline void dyn_inertia_inverse(const float* __restrict__ inertia, double* Iinv) {
  double I[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) I[i] = (double)inertia[i];
  const double c00 = I[4] * I[8] - I[5] * I[7], c01 = I[5] * I[6] - I[3] * I[8],
               c02 = I[3] * I[7] - I[4] * I[6];
  const double det = I[0] * c00 + I[1] * c01 + I[2] * c02;
  const double id = 1.0 / det;
  Iinv[0] = c00 * id;
  Iinv[1] = (I[2] * I[7] - I[1] * I[8]) * id;
  Iinv[2] = (I[1] * I[5] - I[2] * I[4]) * id;
  Iinv[3] = c01 * id;
  Iinv[4] = (I[0] * I[8] - I[2] * I[6]) * id;
  Iinv[5] = (I[2] * I[3] - I[0] * I[5]) * id;
  Iinv[6] = c02 * id;
  Iinv[7] = (I[1] * I[6] - I[0] * I[7]) * id;
  Iinv[8] = (I[0] * I[4] - I[1] * I[3]) * id;
}

// (1/N) sum_k col5[k][5] of a robot's [N][12] fp32 rows, dynamics_kernel's way: lanes 0..N-1 load
// one step each into ys, every lane sums the 16 slots in order.  Ends with ys readable; the
// caller keeps a barrier between two calls on the same ys.
__device__ inline double dyn_mean_yaw(const float* __restrict__ rows, int N, int lane, double* ys) {
  if (lane < 16) ys[lane] = (lane < N) ? (double)rows[lane * 12 + 5] : 0.0;
  __syncthreads();
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) sum += ys[k];
  return sum / N;
}

// C = A B, C = A' B, C = A B' of row-major 3x3s
__device__ inline void dyn_mul(const double* A, const double* Bm, double* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      C[i * 3 + j] = A[i * 3] * Bm[j] + A[i * 3 + 1] * Bm[3 + j] + A[i * 3 + 2] * Bm[6 + j];
}
__device__ inline void dyn_mul_tn(const double* A, const double* Bm, double* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      C[i * 3 + j] = A[i] * Bm[j] + A[3 + i] * Bm[3 + j] + A[6 + i] * Bm[6 + j];
}
__device__ inline void dyn_mul_nt(const double* A, const double* Bm, double* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      C[i * 3 + j] = A[i * 3] * Bm[j * 3] + A[i * 3 + 1] * Bm[j * 3 + 1] + A[i * 3 + 2] * Bm[j * 3 + 2];
}

// the sum over the wave's 64 lanes in one fixed order, the same bits in every lane
__device__ inline double dyn_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ void __launch_bounds__(64) vjp_dynamics_kernel(int N, double dt, int64_t B, DynVjpArgs a) {
  __shared__ __attribute__((aligned(16))) double gb[16 * kDynGradStride];
  __shared__ double ys[16];
  const int lane = threadIdx.x;
  const double h2 = 0.5 * dt * dt;
  // what is wanted, and the 3-row groups of g_Bd's blocks it reads (all wave-uniform)
  const bool want_m = a.g_mass != nullptr, want_i = a.g_inertia != nullptr,
             want_r = a.g_r_feet != nullptr, want_y = a.g_yaw != nullptr;
  const bool want_w = want_i || want_r;                  // needs M, the gradient in W
  const bool have = a.g_Bd != nullptr;
  const bool rows02 = have && want_m;                    // G0, G2
  const bool rows1 = have && (want_w || want_y);         // G1
  const bool rows3 = have && want_w;                     // G3
  const bool active = lane < 4 * N;
  const int k = lane >> 2, l = lane & 3;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    if (have) {  // g_Bd[b] -> LDS, 16 bytes per lane, only the row groups that are read
      const double2* src = reinterpret_cast<const double2*>(a.g_Bd + b * (int64_t)N * 144);
#pragma unroll 6
      for (int e = lane; e < N * 72; e += 64) {
        const int kk = e / 72, j = e - kk * 72, q = j / 18;
        const bool need = (q == 1) ? rows1 : (q == 3) ? rows3 : rows02;
        if (need) reinterpret_cast<double2*>(gb + kk * kDynGradStride)[j] = src[e];
      }
    }
    // per-robot scalars, redundantly per lane (uniform loads): 1/m, I^-1, R_z(yaw_avg)'
    const double minv = 1.0 / (double)a.mass[b];
    double J[9];
    dyn_inertia_inverse(a.inertia + b * 9, J);
    const double yaw = dyn_mean_yaw(a.xref + b * (int64_t)N * 12, N, lane, ys);  // (barrier: gb too)
    const double cy = cos(yaw), sy = sin(yaw);
    const double Rt[9] = {cy, sy, 0.0, -sy, cy, 0.0, 0.0, 0.0, 1.0};

    const double* blk = gb + k * kDynGradStride + 3 * l;   // this lane's 12 x 3 block, row stride 12
    if (want_m) {  // g_minv = sum_kl h2 tr G0 + dt tr G2
      double p = 0.0;
      if (rows02 && active)
        p = h2 * (blk[0] + blk[13] + blk[26]) + dt * (blk[72] + blk[85] + blk[98]);
      const double g_minv = dyn_wave_sum(p);
      if (lane == 0) a.g_mass[b] = -g_minv * (minv * minv);
    }
    if (want_w || want_y) {
      double G1[9], S[9], W[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) G1[i] = 0.0;
      double rx = 0.0, ry = 0.0, rz = 0.0;
      if (active) {
        const float* r = a.r_feet + ((b * N + k) * 4 + l) * 3;
        rx = r[0], ry = r[1], rz = r[2];
        if (rows1) {
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) G1[i * 3 + j] = blk[(3 + i) * 12 + j];
        }
      }
      S[0] = 0.0, S[1] = -rz, S[2] = ry, S[3] = rz, S[4] = 0.0, S[5] = -rx, S[6] = -ry, S[7] = rx,
      S[8] = 0.0;
      dyn_mul(J, S, W);
      if (want_w) {
        double M[9], T[9];  // M = dt G3 + h2 Rt' G1, the gradient in W
        dyn_mul_tn(Rt, G1, T);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const double g3 = (rows3 && active) ? blk[(9 + i) * 12 + j] : 0.0;
            M[i * 3 + j] = dt * g3 + h2 * T[i * 3 + j];
          }
        if (want_r && active) {  // g_S = J' M; r enters S antisymmetrically
          double gS[9];
          dyn_mul_tn(J, M, gS);
          double* o = a.g_r_feet + ((b * N + k) * 4 + l) * 3;
          o[0] = gS[7] - gS[5];
          o[1] = gS[2] - gS[6];
          o[2] = gS[3] - gS[1];
        }
        if (want_i) {  // g_J = sum_kl M S', g_inertia = -J' g_J J'
          double gJ[9], U[9], gI[9];
          dyn_mul_nt(M, S, gJ);
#pragma unroll
          for (int i = 0; i < 9; ++i) gJ[i] = dyn_wave_sum(active ? gJ[i] : 0.0);
          dyn_mul_tn(J, gJ, U);
          dyn_mul_nt(U, J, gI);
          if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) a.g_inertia[b * 9 + i] = -gI[i];
          }
        }
      }
      if (want_y) {  // g_Rt[0:2, 0:2] = dt g_Ad[3:5, 9:11] + h2 sum_kl (G1 W')[0:2, 0:2]
        double gR[4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const double p = G1[i * 3] * W[j * 3] + G1[i * 3 + 1] * W[j * 3 + 1] +
                             G1[i * 3 + 2] * W[j * 3 + 2];
            const double ga = a.g_Ad ? a.g_Ad[b * 144 + (3 + i) * 12 + 9 + j] : 0.0;
            gR[i * 2 + j] = dt * ga + h2 * dyn_wave_sum(active ? p : 0.0);
          }
        if (lane == 0) a.g_yaw[b] = -sy * gR[0] + cy * gR[1] - cy * gR[2] - sy * gR[3];
      }
    }
    __syncthreads();  // gb and ys are rewritten for the next robot
  }
}

__global__ void __launch_bounds__(64) jvp_dynamics_kernel(int N, double dt, int64_t B, DynJvpArgs a) {
  __shared__ __attribute__((aligned(16))) float bd[16 * 144];
  __shared__ double ys[16], dys[16];
  const int lane = threadIdx.x;
  const double h2 = 0.5 * dt * dt;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    // per-robot scalars and their tangents, redundantly per lane (uniform loads)
    const double minv = 1.0 / (double)a.mass[b];
    const double dminv = -(a.d_mass ? (double)a.d_mass[b] : 0.0) * (minv * minv);
    double J[9], dI[9], T[9], dJ[9];
    dyn_inertia_inverse(a.inertia + b * 9, J);
#pragma unroll
    for (int i = 0; i < 9; ++i) dI[i] = a.d_inertia ? (double)a.d_inertia[b * 9 + i] : 0.0;
    dyn_mul(J, dI, T);
    dyn_mul(T, J, dJ);
#pragma unroll
    for (int i = 0; i < 9; ++i) dJ[i] = -dJ[i];          // dJ = -J dI J
    const double yaw = dyn_mean_yaw(a.xref + b * (int64_t)N * 12, N, lane, ys);
    const double dyaw = a.d_xref ? dyn_mean_yaw(a.d_xref + b * (int64_t)N * 12, N, lane, dys) : 0.0;
    const double cy = cos(yaw), sy = sin(yaw);
    const double Rt[9] = {cy, sy, 0.0, -sy, cy, 0.0, 0.0, 0.0, 1.0};
    const double dRt[9] = {-sy * dyaw, cy * dyaw, 0.0, -cy * dyaw, -sy * dyaw, 0.0, 0.0, 0.0, 0.0};

    if (a.d_Bd) {
      // d_Bd_k column block of leg l (12 x 3), lane = 4k + l
      if (lane < 4 * N) {
        const int k = lane >> 2, l = lane & 3;
        const int64_t at = ((b * N + k) * 4 + l) * 3;
        const float* r = a.r_feet + at;
        const double rx = r[0], ry = r[1], rz = r[2];
        double dx = 0.0, dy = 0.0, dz = 0.0;
        if (a.d_r_feet) dx = a.d_r_feet[at], dy = a.d_r_feet[at + 1], dz = a.d_r_feet[at + 2];
        const double S[9] = {0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0};
        const double dS[9] = {0.0, -dz, dy, dz, 0.0, -dx, -dy, dx, 0.0};
        double W[9], dW[9], dV[9], P[9];
        dyn_mul(J, S, W);
        dyn_mul(dJ, S, dW);
        dyn_mul(J, dS, P);
#pragma unroll
        for (int i = 0; i < 9; ++i) dW[i] += P[i];       // dW = dJ S + J dS
        dyn_mul(dRt, W, dV);
        dyn_mul(Rt, dW, P);
#pragma unroll
        for (int i = 0; i < 9; ++i) dV[i] += P[i];       // dV = dRt W + Rt dW
        float* blk = bd + k * 144 + 3 * l;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double e = (i == c) ? dminv : 0.0;
            blk[i * 12 + c] = (float)(h2 * e);
            blk[(3 + i) * 12 + c] = (float)(h2 * dV[i * 3 + c]);
            blk[(6 + i) * 12 + c] = (float)(dt * e);
            blk[(9 + i) * 12 + c] = (float)(dt * dW[i * 3 + c]);
          }
      }
      __syncthreads();
      float4* bo = reinterpret_cast<float4*>(a.d_Bd + b * (int64_t)N * 144);
      const float4* bs = reinterpret_cast<const float4*>(bd);
      for (int e = lane; e < N * 36; e += 64) bo[e] = bs[e];
    }
    if (a.d_Ad && lane < 36) {  // d_Ad = dt dRt in [3:5, 9:11] (flat 45, 46, 57, 58), 0 elsewhere
      float4 v;
      float* pv = reinterpret_cast<float*>(&v);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int o = 4 * lane + q;
        const double d = o == 45 ? dRt[0] : o == 46 ? dRt[1] : o == 57 ? dRt[3] : dRt[4];
        pv[q] = (o == 45 || o == 46 || o == 57 || o == 58) ? (float)(dt * d) : 0.f;
      }
      reinterpret_cast<float4*>(a.d_Ad + b * 144)[lane] = v;
    }
    __syncthreads();  // bd, ys and dys are rewritten for the next robot
  }
}

}  // namespace cmpc
