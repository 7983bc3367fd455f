// cmpc_sim_grad.hip -- reverse- and forward-mode derivatives of cmpc_sim.hip's rigid-body plant
// (cmpc_srb_vjp_run / cmpc_srb_jvp_run, include/cmpc.h), for a batch of robots.
//
// The function differentiated is the plant's documented model in fp64 on the fp32 inputs widened
// exactly (include/cmpc.h spells it out), not srb_kernel's fp32 arithmetic.  The stance pattern and
// the landings depend on t_now, gait and contact_state alone: both kernels first replay the
// substep times (repeated addition of dt from t_now, stance_at's own arithmetic) into one 64-bit
// word per leg, bit k = in stance at substep k, and every later pass reads masks and landings off
// those words.  Time is never stepped backward.
//
// srb_jvp_kernel: one thread per robot, primal and tangent advance together, no tape.
//
// srb_vjp_kernel: one thread per robot, 64-thread blocks, and a two-level tape in LDS, laid out
// [slot][component][lane] so that a wave's access to one component is 64 consecutive doubles.  A
// forward pass stores a checkpoint (state and feet, 24 doubles) at every kSrbSeg-th substep but the
// first, whose state is the input; then, from the last segment to the first, the segment is re-run
// from its checkpoint with each substep's start state (12 doubles) written to an 8-slot tape, and
// swept backward.  The kernel is instantiated for the longest call (7 checkpoints, 135,168 B per
// block, one block per CU) and for nsub <= 24 (2 checkpoints, 73,728 B, two blocks per CU).  A lane
// only ever touches its own column of the tape, so the kernel has no barrier.  Feet are not taped:
// in the backward sweep a foot changes only where the sweep crosses a landing, and there it is
// restored from the previous landing's taped state or from the checkpoint.
//
// Every loop over legs, axes or matrix entries is fully unrolled so that the per-thread arrays
// stay in registers; only the tape is indexed at run time, and it is LDS.
//
// This file is compiled as part of cmpc_host.hip (single translation unit), after cmpc_traj.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cmpc {

constexpr int kSrbSeg = 8;                                       // substeps per tape segment
// checkpoints kept in LDS (segment 0 starts from the inputs): of the longest call, and of the short
// calls that get a smaller tape and with it two blocks per CU
constexpr int kSrbStoredMax = CMPC_SRB_GRAD_MAX_NSUB / kSrbSeg - 1;
constexpr int kSrbStoredShort = 2;
constexpr int kSrbShortNsub = (kSrbStoredShort + 1) * kSrbSeg;
// doubles of LDS per block of 64 robots
constexpr int srb_tape_doubles(int stored) { return (stored * 24 + kSrbSeg * 12) * 64; }
static_assert(CMPC_SRB_GRAD_MAX_NSUB == 64, "the stance words hold one bit per substep");
static_assert(srb_tape_doubles(kSrbStoredMax) * 8 <= 160 * 1024, "the tape must fit one CU's LDS");
static_assert(srb_tape_doubles(kSrbStoredShort) * 8 * 2 <= 160 * 1024, "two short blocks per CU");

struct SrbIn {
  const double *t_now, *gait;
  const float *mass, *inertia_body, *force;
  int64_t force_stride;
  const float *hip, *x, *feet;
  const uint8_t* contact_state;
};

struct SrbVjpArgs {
  SrbIn in;
  const double *g_x_out, *g_feet_out;
  double *g_x, *g_feet, *g_force, *g_mass, *g_inertia_body;
};

struct SrbJvpArgs {
  SrbIn in;
  const float *d_x, *d_feet, *d_force, *d_mass, *d_inertia_body;
  float *d_x_out, *d_feet_out;
};

// the contact schedule of one robot: bit k of stance[l] = leg l in stance at substep k, of land[l]
// = it lands there (in stance, and not at the substep before; before substep 0: contact_state)
struct SrbSchedule {
  uint64_t stance[4], land[4];
};

__device__ inline SrbSchedule srb_schedule(const SrbIn& in, int64_t b, int nsub, double dt) {
  SrbSchedule c;
  const double* gt = in.gait + b * 6;
  const double period = gt[0], duty = gt[1];
  const double off[4] = {gt[2], gt[3], gt[4], gt[5]};
#pragma unroll
  for (int l = 0; l < 4; ++l) c.stance[l] = 0;
  double t = in.t_now[b];
  for (int k = 0; k < nsub; ++k) {
#pragma unroll
    for (int l = 0; l < 4; ++l)
      if (stance_at(t, period, duty, off[l])) c.stance[l] |= 1ull << k;
    t += dt;
  }
  const unsigned before = in.contact_state[b];
#pragma unroll
  for (int l = 0; l < 4; ++l)
    c.land[l] = c.stance[l] & ~((c.stance[l] << 1) | (uint64_t)((before >> l) & 1u));
  return c;
}

__device__ inline unsigned srb_bits(const uint64_t (&w)[4], int k) {
  unsigned m = 0;
#pragma unroll
  for (int l = 0; l < 4; ++l) m |= (unsigned)((w[l] >> k) & 1ull) << l;
  return m;
}

// what does not change over the substeps
struct SrbConst {
  double m, h, half_ts;
  double Ib[9], f[12], hx[4], hy[4];
};

__device__ inline SrbConst srb_const(const SrbIn& in, int64_t b, double dt) {
  SrbConst c;
  c.m = in.mass[b];
  c.h = dt;
  c.half_ts = (in.gait[b * 6 + 1] * in.gait[b * 6]) / 2.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) c.Ib[i] = in.inertia_body[b * 9 + i];
#pragma unroll
  for (int i = 0; i < 12; ++i) c.f[i] = in.force[b * in.force_stride + i];
#pragma unroll
  for (int l = 0; l < 4; ++l) c.hx[l] = in.hip[l * 3], c.hy[l] = in.hip[l * 3 + 1];
  return c;
}

// a 3 x 3 product C = A op(B), row-major
__device__ inline void srb_mm(const double* A, const double* Bm, bool bt, double* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      C[i * 3 + j] = bt ? A[i * 3] * Bm[j * 3] + A[i * 3 + 1] * Bm[j * 3 + 1] + A[i * 3 + 2] * Bm[j * 3 + 2]
                        : A[i * 3] * Bm[j] + A[i * 3 + 1] * Bm[3 + j] + A[i * 3 + 2] * Bm[6 + j];
}

__device__ inline void srb_mv(const double* A, const double* v, double* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = A[i * 3] * v[0] + A[i * 3 + 1] * v[1] + A[i * 3 + 2] * v[2];
}

__device__ inline void srb_mtv(const double* A, const double* v, double* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2];
}

__device__ inline void srb_cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// a landing leg's foot from the substep's starting p, yaw and v
__device__ inline void srb_touchdown(const SrbConst& c, int l, double px, double py, double cy,
                                     double sy, double vx, double vy, double* foot) {
  foot[0] = px + (cy * c.hx[l] - sy * c.hy[l]) + vx * c.half_ts;
  foot[1] = py + (sy * c.hx[l] + cy * c.hy[l]) + vy * c.half_ts;
  foot[2] = 0.0;
}

__device__ inline void srb_land(const SrbConst& c, unsigned land, const double* s, double* ft) {
  if (!land) return;
  const double cy = cos(s[5]), sy = sin(s[5]);
#pragma unroll
  for (int l = 0; l < 4; ++l)
    if (land & (1u << l)) srb_touchdown(c, l, s[0], s[1], cy, sy, s[6], s[7], ft + 3 * l);
}

// what a substep's start state gives every pass
struct SrbGeom {
  double cr, sr, cp, sp, cy, sy;
  double R[9], Iw[9], Inv[9];
  double F[3], T[3], y[3], al[3];
};

__device__ inline void srb_geom(const SrbConst& c, const double* s, const double* ft,
                                unsigned mask, SrbGeom& q) {
  q.cr = cos(s[3]), q.sr = sin(s[3]), q.cp = cos(s[4]), q.sp = sin(s[4]);
  q.cy = cos(s[5]), q.sy = sin(s[5]);
  q.R[0] = q.cy * q.cp, q.R[1] = q.cy * q.sp * q.sr - q.sy * q.cr, q.R[2] = q.cy * q.sp * q.cr + q.sy * q.sr;
  q.R[3] = q.sy * q.cp, q.R[4] = q.sy * q.sp * q.sr + q.cy * q.cr, q.R[5] = q.sy * q.sp * q.cr - q.cy * q.sr;
  q.R[6] = -q.sp, q.R[7] = q.cp * q.sr, q.R[8] = q.cp * q.cr;
  double RI[9];
  srb_mm(q.R, c.Ib, false, RI);
  srb_mm(RI, q.R, true, q.Iw);
#pragma unroll
  for (int i = 0; i < 3; ++i) q.F[i] = 0.0, q.T[i] = 0.0;
#pragma unroll
  for (int l = 0; l < 4; ++l)
    if (mask & (1u << l)) {
      const double r[3] = {ft[3 * l] - s[0], ft[3 * l + 1] - s[1], ft[3 * l + 2] - s[2]};
      double rxf[3];
      srb_cross(r, c.f + 3 * l, rxf);
#pragma unroll
      for (int i = 0; i < 3; ++i) q.F[i] += c.f[3 * l + i], q.T[i] += rxf[i];
    }
  srb_mv(q.Iw, s + 9, q.y);
  double gyro[3], rhs[3];
  srb_cross(s + 9, q.y, gyro);
#pragma unroll
  for (int i = 0; i < 3; ++i) rhs[i] = q.T[i] - gyro[i];
  // the general inverse (adjugate over the determinant)
  const double* A = q.Iw;
  const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8],
               c02 = A[3] * A[7] - A[4] * A[6];
  const double id = 1.0 / (A[0] * c00 + A[1] * c01 + A[2] * c02);
  q.Inv[0] = c00 * id, q.Inv[1] = (A[2] * A[7] - A[1] * A[8]) * id, q.Inv[2] = (A[1] * A[5] - A[2] * A[4]) * id;
  q.Inv[3] = c01 * id, q.Inv[4] = (A[0] * A[8] - A[2] * A[6]) * id, q.Inv[5] = (A[2] * A[3] - A[0] * A[5]) * id;
  q.Inv[6] = c02 * id, q.Inv[7] = (A[1] * A[6] - A[0] * A[7]) * id, q.Inv[8] = (A[0] * A[4] - A[1] * A[3]) * id;
  srb_mv(q.Inv, rhs, q.al);
}

// v and w first, then p and rpy with the new v and w (the rate map's trigonometry is the start's)
__device__ inline void srb_advance(const SrbConst& c, const SrbGeom& q, double* s) {
  s[6] += c.h * (q.F[0] / c.m);
  s[7] += c.h * (q.F[1] / c.m);
  s[8] += c.h * (q.F[2] / c.m - 9.81);
#pragma unroll
  for (int i = 0; i < 3; ++i) s[9 + i] += c.h * q.al[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) s[i] += c.h * s[6 + i];
  const double rd = (q.cy * s[9] + q.sy * s[10]) / q.cp;
  const double pd = -q.sy * s[9] + q.cy * s[10];
  s[3] += c.h * rd;
  s[4] += c.h * pd;
  s[5] += c.h * (s[11] + q.sp * rd);
}

// dR = hat(u) R for a change de of rpy: u = dyaw e_z + dpitch R_z e_y + droll R_z R_y e_x
__device__ inline void srb_rot_axis(const SrbGeom& q, const double* de, double* u) {
  u[0] = -q.sy * de[1] + q.cy * q.cp * de[0];
  u[1] = q.cy * de[1] + q.sy * q.cp * de[0];
  u[2] = de[2] - q.sp * de[0];
}

__global__ void __launch_bounds__(64) srb_jvp_kernel(int64_t B, int nsub, double dt, SrbJvpArgs a) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const SrbSchedule sch = srb_schedule(a.in, b, nsub, dt);
  const SrbConst c = srb_const(a.in, b, dt);
  double s[12], ft[12], ds[12], dft[12], df[12], dIb[9];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    s[i] = a.in.x[b * 12 + i];
    ft[i] = a.in.feet[b * 12 + i];
    ds[i] = a.d_x ? (double)a.d_x[b * 12 + i] : 0.0;
    dft[i] = a.d_feet ? (double)a.d_feet[b * 12 + i] : 0.0;
    df[i] = a.d_force ? (double)a.d_force[b * 12 + i] : 0.0;
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) dIb[i] = a.d_inertia_body ? (double)a.d_inertia_body[b * 9 + i] : 0.0;
  const double dm = a.d_mass ? (double)a.d_mass[b] : 0.0;
  SrbGeom q;
  for (int k = 0; k < nsub; ++k) {
    const unsigned mask = srb_bits(sch.stance, k), land = srb_bits(sch.land, k);
    if (land) {
      const double cy = cos(s[5]), sy = sin(s[5]);
#pragma unroll
      for (int l = 0; l < 4; ++l)
        if (land & (1u << l)) {
          srb_touchdown(c, l, s[0], s[1], cy, sy, s[6], s[7], ft + 3 * l);
          dft[3 * l] = ds[0] - (sy * c.hx[l] + cy * c.hy[l]) * ds[5] + ds[6] * c.half_ts;
          dft[3 * l + 1] = ds[1] + (cy * c.hx[l] - sy * c.hy[l]) * ds[5] + ds[7] * c.half_ts;
          dft[3 * l + 2] = 0.0;
        }
    }
    srb_geom(c, s, ft, mask, q);
    // dIw = hat(u) Iw - Iw hat(u) + R dIb R'
    double u[3], dIw[9], RI[9];
    srb_rot_axis(q, ds + 3, u);
    srb_mm(q.R, dIb, false, RI);
    srb_mm(RI, q.R, true, dIw);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double col[3] = {q.Iw[j], q.Iw[3 + j], q.Iw[6 + j]};
      double uc[3], ru[3];
      srb_cross(u, col, uc);
      srb_cross(q.Iw + 3 * j, u, ru);  // row j of Iw hat(u)
#pragma unroll
      for (int i = 0; i < 3; ++i) dIw[i * 3 + j] += uc[i], dIw[j * 3 + i] -= ru[i];
    }
    double dF[3] = {0.0, 0.0, 0.0}, dT[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int l = 0; l < 4; ++l)
      if (mask & (1u << l)) {
        const double r[3] = {ft[3 * l] - s[0], ft[3 * l + 1] - s[1], ft[3 * l + 2] - s[2]};
        const double dr[3] = {dft[3 * l] - ds[0], dft[3 * l + 1] - ds[1], dft[3 * l + 2] - ds[2]};
        double t1[3], t2[3];
        srb_cross(dr, c.f + 3 * l, t1);
        srb_cross(r, df + 3 * l, t2);
#pragma unroll
        for (int i = 0; i < 3; ++i) dF[i] += df[3 * l + i], dT[i] += t1[i] + t2[i];
      }
    // dal = Iw^-1 (dT - dw x y - w x (dIw w + Iw dw) - dIw al)
    double dy[3], t1[3], t2[3], t3[3], t4[3], rhs[3], dal[3];
    srb_mv(dIw, s + 9, dy);
    srb_mv(q.Iw, ds + 9, t1);
#pragma unroll
    for (int i = 0; i < 3; ++i) dy[i] += t1[i];
    srb_cross(ds + 9, q.y, t2);
    srb_cross(s + 9, dy, t3);
    srb_mv(dIw, q.al, t4);
#pragma unroll
    for (int i = 0; i < 3; ++i) rhs[i] = dT[i] - t2[i] - t3[i] - t4[i];
    srb_mv(q.Inv, rhs, dal);
    const double de[3] = {ds[3], ds[4], ds[5]};  // the start's, for the rate map
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      ds[6 + i] += c.h * (dF[i] / c.m - q.F[i] * dm / (c.m * c.m));
      ds[9 + i] += c.h * dal[i];
      ds[i] += c.h * ds[6 + i];
    }
    srb_advance(c, q, s);
    // the rates of the new w, E taken at the start's rpy
    const double n = q.cy * s[9] + q.sy * s[10];
    const double rd = n / q.cp, pd = -q.sy * s[9] + q.cy * s[10];
    const double drd = (q.cy * ds[9] + q.sy * ds[10]) / q.cp + (pd / q.cp) * de[2] + rd * (q.sp / q.cp) * de[1];
    const double dpd = -q.sy * ds[9] + q.cy * ds[10] - n * de[2];
    const double dyd = ds[11] + q.sp * drd + q.cp * rd * de[1];
    ds[3] += c.h * drd;
    ds[4] += c.h * dpd;
    ds[5] += c.h * dyd;
  }
  if (a.d_x_out) {
#pragma unroll
    for (int i = 0; i < 12; ++i) a.d_x_out[b * 12 + i] = (float)ds[i];
  }
  if (a.d_feet_out) {
#pragma unroll
    for (int i = 0; i < 12; ++i) a.d_feet_out[b * 12 + i] = (float)dft[i];
  }
}

// kStored: the checkpoints the block's LDS holds; nsub <= (kStored + 1) kSrbSeg
template <int kStored>
__global__ void __launch_bounds__(64) srb_vjp_kernel(int64_t B, int nsub, double dt, SrbVjpArgs a) {
  __shared__ double lds[srb_tape_doubles(kStored)];
  const int lane = threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x * 64 + lane;
  if (b >= B) return;  // (no barrier below: a lane touches its own column of the tape only)
  double* ckpt = lds + lane;                      // [segment - 1][24][lane]
  double* tape = lds + kStored * 24 * 64 + lane;  // [slot][12][lane]
  const SrbSchedule sch = srb_schedule(a.in, b, nsub, dt);
  const SrbConst c = srb_const(a.in, b, dt);
  const bool need_m = a.g_mass != nullptr, need_Ib = a.g_inertia_body != nullptr;
  double s[12], ft[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) s[i] = a.in.x[b * 12 + i], ft[i] = a.in.feet[b * 12 + i];
  SrbGeom q;
  // forward to the last segment's start, a checkpoint at the start of every segment but the first
  const int nseg = (nsub + kSrbSeg - 1) / kSrbSeg;
  for (int k = 0; k < (nseg - 1) * kSrbSeg; ++k) {
    srb_land(c, srb_bits(sch.land, k), s, ft);
    srb_geom(c, s, ft, srb_bits(sch.stance, k), q);
    srb_advance(c, q, s);
    if ((k + 1) % kSrbSeg == 0) {
      double* o = ckpt + ((k + 1) / kSrbSeg - 1) * 24 * 64;
#pragma unroll
      for (int i = 0; i < 12; ++i) o[i * 64] = s[i], o[(12 + i) * 64] = ft[i];
    }
  }
  double g[12], gc[12], gf[12], gIb[9], gm = 0.0;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    g[i] = a.g_x_out ? a.g_x_out[b * 12 + i] : 0.0;
    gc[i] = a.g_feet_out ? a.g_feet_out[b * 12 + i] : 0.0;
    gf[i] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) gIb[i] = 0.0;
  for (int seg = nseg - 1; seg >= 0; --seg) {
    const int k0 = seg * kSrbSeg, k1 = min(nsub, k0 + kSrbSeg);
    const double* ck = ckpt + (seg - 1) * 24 * 64;  // (segment 0 starts from the inputs)
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      s[i] = seg ? ck[i * 64] : (double)a.in.x[b * 12 + i];
      ft[i] = seg ? ck[(12 + i) * 64] : (double)a.in.feet[b * 12 + i];
    }
    // the segment again, each substep's start state onto the tape
    for (int k = k0; k < k1; ++k) {
      double* o = tape + (k - k0) * 12 * 64;
#pragma unroll
      for (int i = 0; i < 12; ++i) o[i * 64] = s[i];
      srb_land(c, srb_bits(sch.land, k), s, ft);
      if (k + 1 < k1) {  // (the state after the last substep is not needed)
        srb_geom(c, s, ft, srb_bits(sch.stance, k), q);
        srb_advance(c, q, s);
      }
    }
    // and backward; ft holds the feet as substep k uses them
    for (int k = k1 - 1; k >= k0; --k) {
      const double* o = tape + (k - k0) * 12 * 64;
#pragma unroll
      for (int i = 0; i < 12; ++i) s[i] = o[i * 64];
      const unsigned mask = srb_bits(sch.stance, k), land = srb_bits(sch.land, k);
      srb_geom(c, s, ft, mask, q);
      const double wn[3] = {s[9] + c.h * q.al[0], s[10] + c.h * q.al[1], s[11] + c.h * q.al[2]};
      // rpy' = rpy + h E(rpy) w'
      {
        const double ga = c.h * g[3], gb = c.h * g[4], gy = c.h * g[5];
        const double n = q.cy * wn[0] + q.sy * wn[1];
        const double rd = n / q.cp, pd = -q.sy * wn[0] + q.cy * wn[1];
        const double grd = ga + q.sp * gy;
        g[9] += grd * q.cy / q.cp - q.sy * gb;
        g[10] += grd * q.sy / q.cp + q.cy * gb;
        g[11] += gy;
        g[4] += grd * rd * (q.sp / q.cp) + gy * q.cp * rd;
        g[5] += grd * (pd / q.cp) - gb * n;
      }
      // p' = p + h v';  v' = v + h (F / m + g)
      double gF[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        g[6 + i] += c.h * g[i];
        gF[i] = (c.h / c.m) * g[6 + i];
      }
      if (need_m) gm -= c.h * (q.F[0] * g[6] + q.F[1] * g[7] + q.F[2] * g[8]) / (c.m * c.m);
      // w' = w + h al,  al = Iw^-1 (T - w x y),  y = Iw w
      const double gal[3] = {c.h * g[9], c.h * g[10], c.h * g[11]};
      double qv[3], t1[3], gy3[3], t2[3], gIw[9];
      srb_mtv(q.Inv, gal, qv);     // the adjoint of the right-hand side, and of T
      srb_cross(qv, q.y, t1);      // w x y in w
      srb_cross(s + 9, qv, gy3);   // w x y in y
      srb_mtv(q.Iw, gy3, t2);
#pragma unroll
      for (int i = 0; i < 3; ++i) g[9 + i] += t1[i] + t2[i];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) gIw[i * 3 + j] = gy3[i] * s[9 + j] - qv[i] * q.al[j];
      // Iw = R Ib R': rpy through dR = hat(u) R, which needs M = gIw Iw' + gIw' Iw only
      {
        double M1[9], M[9];
        srb_mm(gIw, q.Iw, true, M1);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j)
            M[i * 3 + j] = M1[i * 3 + j] + gIw[i] * q.Iw[j] + gIw[3 + i] * q.Iw[3 + j] + gIw[6 + i] * q.Iw[6 + j];
        const double k0v = M[7] - M[5], k1v = M[2] - M[6], k2v = M[3] - M[1];
        g[3] += q.cy * q.cp * k0v + q.sy * q.cp * k1v - q.sp * k2v;
        g[4] += -q.sy * k0v + q.cy * k1v;
        g[5] += k2v;
      }
      if (need_Ib) {  // gIb += R' gIw R
        double GR[9];
        srb_mm(gIw, q.R, false, GR);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j)
            gIb[i * 3 + j] += q.R[i] * GR[j] + q.R[3 + i] * GR[3 + j] + q.R[6 + i] * GR[6 + j];
      }
      // F and T over the stance legs
#pragma unroll
      for (int l = 0; l < 4; ++l)
        if (mask & (1u << l)) {
          const double r[3] = {ft[3 * l] - s[0], ft[3 * l + 1] - s[1], ft[3 * l + 2] - s[2]};
          double gr[3], gfl[3];
          srb_cross(c.f + 3 * l, qv, gr);
          srb_cross(qv, r, gfl);
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            gf[3 * l + i] += gF[i] + gfl[i];
            gc[3 * l + i] += gr[i];
            g[i] -= gr[i];
          }
        }
      // the landings of this substep, after its dynamics: the foot's adjoint flows into the start
      // state and the foot goes back to what it was before
      if (land) {
#pragma unroll
        for (int l = 0; l < 4; ++l)
          if (land & (1u << l)) {
            const double gx = gc[3 * l], gy = gc[3 * l + 1];
            g[0] += gx;
            g[1] += gy;
            g[5] += gx * (-q.sy * c.hx[l] - q.cy * c.hy[l]) + gy * (q.cy * c.hx[l] - q.sy * c.hy[l]);
            g[6] += gx * c.half_ts;
            g[7] += gy * c.half_ts;
            gc[3 * l] = 0.0, gc[3 * l + 1] = 0.0, gc[3 * l + 2] = 0.0;
            // the latest landing before k in this segment, else the checkpoint's foot
            const uint64_t inseg = (k > k0) ? (((1ull << (k - k0)) - 1ull) << k0) : 0ull;
            const uint64_t earlier = sch.land[l] & inseg;
            if (earlier) {
              const int j = 63 - __clzll((long long)earlier);
              const double* e = tape + (j - k0) * 12 * 64;
              const double psi = e[5 * 64];
              srb_touchdown(c, l, e[0], e[64], cos(psi), sin(psi), e[6 * 64], e[7 * 64], ft + 3 * l);
            } else {
#pragma unroll
              for (int i = 0; i < 3; ++i)
                ft[3 * l + i] = seg ? ck[(12 + 3 * l + i) * 64] : (double)a.in.feet[b * 12 + 3 * l + i];
            }
          }
      }
    }
  }
  if (a.g_x) {
#pragma unroll
    for (int i = 0; i < 12; ++i) a.g_x[b * 12 + i] = g[i];
  }
  if (a.g_feet) {
#pragma unroll
    for (int i = 0; i < 12; ++i) a.g_feet[b * 12 + i] = gc[i];
  }
  if (a.g_force) {
#pragma unroll
    for (int i = 0; i < 12; ++i) a.g_force[b * 12 + i] = gf[i];
  }
  if (need_m) a.g_mass[b] = gm;
  if (need_Ib) {
#pragma unroll
    for (int i = 0; i < 9; ++i) a.g_inertia_body[b * 9 + i] = gIb[i];
  }
}

}  // namespace cmpc
