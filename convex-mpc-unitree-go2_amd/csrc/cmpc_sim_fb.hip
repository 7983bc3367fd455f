// cmpc_sim_fb.hip -- the rigid-body plant of cmpc_sim.hip with the first-order MPC force law
// applied at every substep and an external wrench (cmpc_srb_step_io_run, include/cmpc.h;
// DESIGN.md 4w).
//
// srb_kernel's substep, restated so that srb_kernel's own code stays as it is, with two additions:
// the forces of a robot that has the law are u = fl32(U0 + K (x_s - x_solve)) at every substep,
// the legs the MPC planned in stance at step 0 clamped into their friction pyramid; and a held
// world wrench at the COM enters F and T.
//
// Layout: one thread per robot, as srb_kernel, 64 robots per block of one wave.  The block first
// copies its robots' K blocks -- one contiguous run of 64 x 1,152 B -- from global memory into LDS
// with 16-byte loads (lane i at byte 16 i: coalesced), once per launch; each thread then reads
// its robot's 144 fp64 entries from LDS.  A robot's row is padded to 145 doubles: the lane stride
// of 290 dwords puts the 32 lanes of a ds_read_b64 group on 32 distinct bank pairs.  Every sum
// runs in one thread in a fixed order; there are no atomics.
//
// This file is compiled as part of cmpc_host.hip (single translation unit).
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cmpc {

constexpr int kSrbFbRobots = 64;  // robots per block (= threads per block): tests/test_gpu_srb_fb.py's R
constexpr int kSrbFbRow = 145;    // doubles per robot in LDS (144 + 1 of padding)

struct SrbFbArgs {
  const double *t_now, *gait;
  const float *mass, *inertia_body, *force;
  int64_t force_stride;
  const float* hip;
  float *x, *feet;
  uint8_t* contact_state;
  const double* K;         // [B][12][12], 16-byte aligned (kLaw only)
  const float* x_solve;    // [B][12]
  const uint8_t* contact;  // [B][4][N]
  const float *mu, *fz_min;  // [B] or NULL: mu0 / fz0
  float mu0, fz0;
  int N;
  const float* wrench;     // [B][6] or NULL
  float* force_out;        // [B][12] or NULL
  uint8_t* fb_status;      // [B] or NULL
};

// kLaw: K is given.  Without it no LDS is used and every robot holds U0.
template <bool kLaw>
__global__ void __launch_bounds__(kSrbFbRobots) srb_feedback_kernel(int64_t B, int nsub, double dt,
                                                                     SrbFbArgs a) {
  __shared__ double Ks[kLaw ? kSrbFbRobots * kSrbFbRow : 1];
  const int64_t b0 = (int64_t)blockIdx.x * kSrbFbRobots;
  const int tid = threadIdx.x;
  const int64_t b = b0 + tid;
  if constexpr (kLaw) {
    // the block's K blocks are contiguous in global memory: 72 double2 per robot, a pair never
    // straddles two robots
    const int nb = (int)(B - b0 < kSrbFbRobots ? B - b0 : kSrbFbRobots);
    const double2* src = reinterpret_cast<const double2*>(a.K + b0 * 144);
    for (int i = tid; i < nb * 72; i += kSrbFbRobots) {
      const double2 v = src[i];
      const int r = i / 72, c = 2 * (i - r * 72);
      Ks[r * kSrbFbRow + c] = v.x;
      Ks[r * kSrbFbRow + c + 1] = v.y;
    }
    __syncthreads();
  }
  if (b >= B) return;
  const double* Kb = &Ks[kLaw ? tid * kSrbFbRow : 0];
  float s[12], ft[4][3], f0[4][3], f[4][3], xs[12];
  for (int i = 0; i < 12; ++i) s[i] = a.x[b * 12 + i];
  for (int l = 0; l < 4; ++l)
    for (int c = 0; c < 3; ++c) {
      ft[l][c] = a.feet[(b * 4 + l) * 3 + c];
      f0[l][c] = a.force[b * a.force_stride + 3 * l + c];
      f[l][c] = f0[l][c];
    }
  // the law: K finite, mu and fz_min valid by cmpc_solve_io's rules; else the robot holds U0
  bool law = false;
  float mu = a.mu0, fzm = a.fz0;
  uint8_t plan_stance = 0;  // bit l: the MPC's step 0 has leg l in stance
  if constexpr (kLaw) {
    if (a.mu) mu = a.mu[b];
    if (a.fz_min) fzm = a.fz_min[b];
    law = isfinite(mu) && mu > 0.f && isfinite(fzm);
    bool finite = true;
    for (int i = 0; i < 144; ++i) finite = finite && isfinite(Kb[i]);
    law = law && finite;
    for (int i = 0; i < 12; ++i) xs[i] = a.x_solve[b * 12 + i];
    for (int l = 0; l < 4; ++l)
      if (a.contact[(b * 4 + l) * a.N] != 0) plan_stance |= (uint8_t)(1u << l);
  }
  bool clamped = false;
  float wr[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (a.wrench)
    for (int i = 0; i < 6; ++i) wr[i] = a.wrench[b * 6 + i];
  const float m = a.mass[b];
  float Ib[9];
  for (int i = 0; i < 9; ++i) Ib[i] = a.inertia_body[b * 9 + i];
  const double period = a.gait[b * 6], duty = a.gait[b * 6 + 1];
  const float t_stance = (float)(duty * period);
  uint8_t cmask = a.contact_state[b];
  double t = a.t_now[b];
  const float h = (float)dt;
  for (int it = 0; it < nsub; ++it) {
    // contact state at the substep time; a landing leg is placed under its hip + v t_stance / 2
    const float cr = cosf(s[3]), sr = sinf(s[3]), cp = cosf(s[4]), sp = sinf(s[4]);
    const float cy = cosf(s[5]), sy = sinf(s[5]);
    uint8_t nm = 0;
    for (int l = 0; l < 4; ++l) {
      const bool st = stance_at(t, period, duty, a.gait[b * 6 + 2 + l]);
      if (st) nm |= (uint8_t)(1u << l);
      if (st && !(cmask & (1u << l))) {
        const float hx = a.hip[l * 3], hy = a.hip[l * 3 + 1];
        ft[l][0] = s[0] + cy * hx - sy * hy + s[6] * 0.5f * t_stance;
        ft[l][1] = s[1] + sy * hx + cy * hy + s[7] * 0.5f * t_stance;
        ft[l][2] = 0.f;
      }
    }
    cmask = nm;
    if constexpr (kLaw) {
      if (law) {
        // u = fl32(U0 + K (x_s - x_solve)): the difference in fp32, the row sums in fp64, j = 0 .. 11
        // (all 12 rows advance together, column by column: 12 independent FMA chains and no
        // branch on the leg; each row's own order is j = 0 .. 11 either way)
        double acc[12];
        for (int i = 0; i < 12; ++i) acc[i] = (double)f0[i / 3][i % 3];
        for (int j = 0; j < 12; ++j) {
          const double dj = (double)(s[j] - xs[j]);
          for (int i = 0; i < 12; ++i) acc[i] = fma(Kb[i * 12 + j], dj, acc[i]);
        }
        for (int l = 0; l < 4; ++l) {
          if (!(plan_stance & (1u << l))) continue;  // planned in swing: U0 as it is
          const float u[3] = {(float)acc[3 * l], (float)acc[3 * l + 1], (float)acc[3 * l + 2]};
          // into the friction pyramid: fz first, the tangential bounds from the clamped fz
          const float fz = fmaxf(u[2], fzm);
          const float lim = mu * fz;
          const float fx = fminf(fmaxf(u[0], -lim), lim), fy = fminf(fmaxf(u[1], -lim), lim);
          if ((cmask & (1u << l)) && (fx != u[0] || fy != u[1] || fz != u[2])) clamped = true;
          f[l][0] = fx; f[l][1] = fy; f[l][2] = fz;
        }
      }
    }
    // R = Rz(y) Ry(p) Rx(r); I_w = R I_b R'
    const float R[9] = {cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr,
                        sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr,
                        -sp,     cp * sr,                cp * cr};
    float RI[9], Iw[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j)
        RI[i * 3 + j] = R[i * 3] * Ib[j] + R[i * 3 + 1] * Ib[3 + j] + R[i * 3 + 2] * Ib[6 + j];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j)
        Iw[i * 3 + j] = RI[i * 3] * R[j * 3] + RI[i * 3 + 1] * R[j * 3 + 1] + RI[i * 3 + 2] * R[j * 3 + 2];
    float F[3] = {0.f, 0.f, -9.81f * m}, T[3] = {0.f, 0.f, 0.f};
    for (int l = 0; l < 4; ++l) {
      if (!(cmask & (1u << l))) continue;
      const float rx = ft[l][0] - s[0], ry = ft[l][1] - s[1], rz = ft[l][2] - s[2];
      F[0] += f[l][0]; F[1] += f[l][1]; F[2] += f[l][2];
      T[0] += ry * f[l][2] - rz * f[l][1];
      T[1] += rz * f[l][0] - rx * f[l][2];
      T[2] += rx * f[l][1] - ry * f[l][0];
    }
    // the external wrench: world force at the COM, world torque about it, whatever the contacts
    for (int i = 0; i < 3; ++i) {
      F[i] += wr[i];
      T[i] += wr[3 + i];
    }
    const float* w = &s[9];
    const float Iww[3] = {Iw[0] * w[0] + Iw[1] * w[1] + Iw[2] * w[2],
                          Iw[3] * w[0] + Iw[4] * w[1] + Iw[5] * w[2],
                          Iw[6] * w[0] + Iw[7] * w[1] + Iw[8] * w[2]};
    const float rhs[3] = {T[0] - (w[1] * Iww[2] - w[2] * Iww[1]),
                          T[1] - (w[2] * Iww[0] - w[0] * Iww[2]),
                          T[2] - (w[0] * Iww[1] - w[1] * Iww[0])};
    // w' = I_w^-1 rhs (adjugate)
    const float c00 = Iw[4] * Iw[8] - Iw[5] * Iw[7], c01 = Iw[5] * Iw[6] - Iw[3] * Iw[8],
                c02 = Iw[3] * Iw[7] - Iw[4] * Iw[6];
    const float id = 1.f / (Iw[0] * c00 + Iw[1] * c01 + Iw[2] * c02);
    const float Inv[9] = {c00 * id, (Iw[2] * Iw[7] - Iw[1] * Iw[8]) * id,
                          (Iw[1] * Iw[5] - Iw[2] * Iw[4]) * id, c01 * id,
                          (Iw[0] * Iw[8] - Iw[2] * Iw[6]) * id, (Iw[2] * Iw[3] - Iw[0] * Iw[5]) * id,
                          c02 * id, (Iw[1] * Iw[6] - Iw[0] * Iw[7]) * id,
                          (Iw[0] * Iw[4] - Iw[1] * Iw[3]) * id};
    // semi-implicit Euler: velocities first, positions with the new velocities
    for (int i = 0; i < 3; ++i) s[6 + i] += h * F[i] / m;
    for (int i = 0; i < 3; ++i)
      s[9 + i] += h * (Inv[i * 3] * rhs[0] + Inv[i * 3 + 1] * rhs[1] + Inv[i * 3 + 2] * rhs[2]);
    for (int i = 0; i < 3; ++i) s[i] += h * s[6 + i];
    // ZYX Euler rates from the world angular velocity
    const float rd = (cy * s[9] + sy * s[10]) / cp;
    const float pd = -sy * s[9] + cy * s[10];
    const float yd = s[11] + sp * rd;
    s[3] += h * rd; s[4] += h * pd; s[5] += h * yd;
    t += dt;
  }
  for (int i = 0; i < 12; ++i) a.x[b * 12 + i] = s[i];
  for (int l = 0; l < 4; ++l)
    for (int c = 0; c < 3; ++c) a.feet[(b * 4 + l) * 3 + c] = ft[l][c];
  a.contact_state[b] = cmask;
  if (a.force_out)
    for (int l = 0; l < 4; ++l)
      for (int c = 0; c < 3; ++c) a.force_out[b * 12 + 3 * l + c] = f[l][c];
  if (a.fb_status) a.fb_status[b] = law ? (clamped ? 2 : 1) : 0;
}

}  // namespace cmpc
