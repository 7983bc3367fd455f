// cmpc_traj_grad.hip -- reverse- and forward-mode derivatives of cmpc_traj.hip's trajectory
// generator (cmpc_traj_vjp_run / cmpc_traj_jvp_run, include/cmpc.h), for a batch of robots.
//
// The function differentiated is what traj_group_kernel evaluates before it rounds, in fp64 on the
// fp32 inputs widened exactly: the clamp of the desired position with its branch held, the
// reference  xref[k] = (pd + vw t_k, 0, 0, psi + wz t_k, vw, 0, 0, 0, wz)  and the levers, each of
// class S (swing: 0), C (stance before any take-off: the current lever) or P (stance after the
// take-off at step j: the touchdown predicted there, a rotation of the hip offset by
// psi + wz t_j plus tau times the body velocity and the yaw-rate cross term).  The classes and j
// depend on t_now and gait alone and come from lever_class, the forward pass's own helper
// (cmpc_traj.hip), so the pattern held fixed is the one the forward pass used, bit for bit.
//
// Both kernels have dynamics_grad's shape: one 64-lane wave per robot, grid-stride over the
// batch, lane = 4k + leg owning one (step, leg), lanes at or past 4N contributing exact zeros.
// With that map a lane owns three contiguous elements of every per-step array: the lever
// [k][leg][0..2] and columns 3 leg .. 3 leg + 2 of xref's row k, so the wave's loads and stores are
// contiguous, 24 B (fp64) or 12 B (fp32) per lane.  They go out as three 8-byte (4-byte) accesses
// per lane and not through an LDS-staged 16-byte pass: a robot moves 3 KB, the three accesses of a
// lane hit the same 64 B lines back to back so every line is fetched from L2 once, and the staged
// form adds two barriers per robot to kernels that otherwise have none.
//
// The per-robot scalars are computed redundantly per lane from uniform loads, except the sin / cos
// pairs, of which a lane evaluates one: lane j < 16 that of the yaw at step j, psi + wz t_j, lanes
// 16, 17, 18 those of roll, pitch and yaw.  The latter are broadcast from those lanes (the same
// bits in every lane) and a class P lane fetches its take-off step's pair with one shuffle.
// vjp_traj_kernel reduces its nine batch-level sums with one xor butterfly of six shuffle steps
// each (32 .. 1) and the three per-leg sums of g_foot_lever with the same butterfly stopped at
// distance 4: fixed trees, the same value in every lane (of the leg), no atomics.  All sums are
// always formed; the outputs only decide what is stored, so an output does not depend on which
// others are asked for.
//
// This file is compiled as part of cmpc_host.hip (single translation unit), after cmpc_traj.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cmpc {

struct TrajIn {
  const float* x0;
  const double* pos_des;
  const float* cmd;
  const double *t_now, *gait;
  const float* hip;
};

struct TrajVjpArgs {
  TrajIn in;
  const double *g_xref, *g_r_feet, *g_yaw, *g_pos_des_out;
  double *g_x0, *g_pos_des, *g_cmd, *g_foot_lever;
};

struct TrajJvpArgs {
  TrajIn in;
  const float* d_x0;
  const double* d_pos_des;
  const float *d_cmd, *d_foot_lever;
  float *d_xref, *d_r_feet;
  double* d_pos_des_out;
};

// what both derivatives read of one robot, the same in every lane but cls, tj, hwx, hwy
struct TrajPoint {
  double sx, sy;                    // 1 where the forward pass clamps the axis, else 0
  double vxb, vyb, wz, tau;
  double c, s, cph, sph, cth, sth;  // cos, sin of yaw, roll, pitch
  double vwx, vwy;
  int cls;                          // lever_class of this lane's (step, leg)
  double tj, hwx, hwy;              // class P: the take-off time and the rotated hip offset
};

__device__ inline double traj_clamped(double pd, double p) {
  bool hit = false;  // the forward pass's two strict tests, the second on the first's result
  if (pd - p > kMaxPosError) pd = p + kMaxPosError, hit = true;
  if (p - pd > kMaxPosError) hit = true;
  return hit ? 1.0 : 0.0;
}

// every lane calls (lever_class ballots, the sin / cos broadcast shuffles)
__device__ inline TrajPoint traj_point(const TrajIn& in, int64_t b, int lane, int N, double dt) {
  TrajPoint q;
  const float* xs = in.x0 + b * 12;
  const float* cm = in.cmd + b * 4;
  const double* gt = in.gait + b * 6;
  q.sx = traj_clamped(in.pos_des[b * 3], (double)xs[0]);
  q.sy = traj_clamped(in.pos_des[b * 3 + 1], (double)xs[1]);
  q.vxb = cm[0], q.vyb = cm[1], q.wz = cm[3];
  const double period = gt[0], duty = gt[1];
  q.tau = ((1.0 - duty) * period + 0.5 * (duty * period)) / 2.0;
  // one sin / cos pair per lane: lane j < 16 the yaw at step j, psi + wz t_j, lanes 16, 17, 18 (and
  // every third lane after them) roll, pitch, yaw
  const double ang = lane < 16 ? (double)xs[5] + q.wz * ((double)(lane + 1) * dt)
                               : (double)xs[3 + (lane - 16) % 3];
  const double ca = cos(ang), sa = sin(ang);
  q.cph = __shfl(ca, 16, 64), q.sph = __shfl(sa, 16, 64);
  q.cth = __shfl(ca, 17, 64), q.sth = __shfl(sa, 17, 64);
  q.c = __shfl(ca, 18, 64), q.s = __shfl(sa, 18, 64);
  q.vwx = q.c * q.vxb - q.s * q.vyb;
  q.vwy = q.s * q.vxb + q.c * q.vyb;
  const int leg = lane & 3;
  q.cls = lever_class(lane, N, dt, in.t_now[b], period, duty, gt[2 + leg]);
  const int j = q.cls >= 0 ? q.cls : 0;  // (every lane shuffles)
  const double cj = __shfl(ca, j, 64), sj = __shfl(sa, j, 64);
  q.tj = 0.0, q.hwx = 0.0, q.hwy = 0.0;
  if (q.cls >= 0) {
    q.tj = (double)(j + 1) * dt;
    const double hx = in.hip[leg * 3], hy = in.hip[leg * 3 + 1];
    q.hwx = cj * hx - sj * hy;
    q.hwy = sj * hx + cj * hy;
  }
  return q;
}

// the sum over the wave's 64 lanes, or over the 16 lanes of a leg (down to distance 4), in one
// fixed order: the same bits in every lane that shares the sum
template <int kLast>
__device__ inline double traj_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= kLast; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ void __launch_bounds__(64) vjp_traj_kernel(int N, double dt, int64_t B, TrajVjpArgs a) {
  const int lane = threadIdx.x;
  const int k = lane >> 2, leg = lane & 3;
  const bool active = lane < 4 * N;
  const double tk = (double)(k + 1) * dt;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const TrajPoint q = traj_point(a.in, b, lane, N, dt);
    // this lane's three elements of G = g_xref (+ g_yaw / N on the yaw column) and H = g_r_feet
    double G0 = 0.0, G1 = 0.0, G2 = 0.0, H0 = 0.0, H1 = 0.0, H2 = 0.0;
    if (active) {
      const int64_t at = (b * N + k) * 12 + 3 * leg;
      if (a.g_xref) G0 = a.g_xref[at], G1 = a.g_xref[at + 1], G2 = a.g_xref[at + 2];
      if (a.g_r_feet) H0 = a.g_r_feet[at], H1 = a.g_r_feet[at + 1], H2 = a.g_r_feet[at + 2];
      if (a.g_yaw && leg == 1) G2 += a.g_yaw[b] / N;
    }
    // the lane's terms of the nine sums: leg 0 holds columns 0-2 of its step, leg 1 columns 3-5,
    // leg 2 columns 6-8, leg 3 columns 9-11
    double p_pdx = 0.0, p_pdy = 0.0, p_z = 0.0, p_vwx = 0.0, p_vwy = 0.0, p_psi = 0.0, p_wz = 0.0,
           p_vbx = 0.0, p_vby = 0.0;
    if (leg == 0) p_pdx = G0, p_pdy = G1, p_z = G2, p_vwx = tk * G0, p_vwy = tk * G1;
    if (leg == 1) p_psi = G2, p_wz = tk * G2;
    if (leg == 2) p_vwx = G0, p_vwy = G1;
    if (leg == 3) p_wz = G2;
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;  // class C: the lever is the current one
    if (q.cls == kLeverCurrent) f0 = H0, f1 = H1, f2 = H2;
    if (q.cls >= 0) {  // class P
      p_z -= H2;
      p_vbx = q.tau * H0, p_vby = q.tau * H1;
      const double g_hwx = H0 + q.wz * q.tau * H1, g_hwy = H1 - q.wz * q.tau * H0;
      const double g_pj = -q.hwy * g_hwx + q.hwx * g_hwy;
      p_wz += q.tau * (-q.hwy * H0 + q.hwx * H1) + q.tj * g_pj;
      p_psi += g_pj;
    }
    const double gp0 = a.g_pos_des_out ? a.g_pos_des_out[b * 3] : 0.0;
    const double gp1 = a.g_pos_des_out ? a.g_pos_des_out[b * 3 + 1] : 0.0;
    const double gp2 = a.g_pos_des_out ? a.g_pos_des_out[b * 3 + 2] : 0.0;
    const double g_pdx = traj_wave_sum<1>(p_pdx) + gp0, g_pdy = traj_wave_sum<1>(p_pdy) + gp1;
    const double g_z = traj_wave_sum<1>(p_z) + gp2;
    const double g_vwx = traj_wave_sum<1>(p_vwx), g_vwy = traj_wave_sum<1>(p_vwy);
    const double g_vbx = traj_wave_sum<1>(p_vbx), g_vby = traj_wave_sum<1>(p_vby);
    const double g_wz = traj_wave_sum<1>(p_wz);
    const double g_psi = traj_wave_sum<1>(p_psi) + (-q.vwy * g_vwx + q.vwx * g_vwy);
    f0 = traj_wave_sum<4>(f0), f1 = traj_wave_sum<4>(f1), f2 = traj_wave_sum<4>(f2);

    if (a.g_x0 && lane < 12) {  // written whole
      const double g_th = -q.sth * q.vxb * g_vbx + q.cth * q.sph * q.vxb * g_vby;
      const double g_ph = (q.sth * q.cph * q.vxb - q.sph * q.vyb) * g_vby;
      const double v = lane == 0 ? q.sx * g_pdx : lane == 1 ? q.sy * g_pdy : lane == 3 ? g_ph
                     : lane == 4 ? g_th : lane == 5 ? g_psi : 0.0;
      a.g_x0[b * 12 + lane] = v;
    }
    if (a.g_pos_des && lane < 3)
      a.g_pos_des[b * 3 + lane] = lane == 0 ? (1.0 - q.sx) * g_pdx : lane == 1 ? (1.0 - q.sy) * g_pdy : 0.0;
    if (a.g_cmd && lane < 4) {
      const double g_vxb = q.c * g_vwx + q.s * g_vwy + q.cth * g_vbx + q.sth * q.sph * g_vby;
      const double g_vyb = -q.s * g_vwx + q.c * g_vwy + q.cph * g_vby;
      a.g_cmd[b * 4 + lane] = lane == 0 ? g_vxb : lane == 1 ? g_vyb : lane == 2 ? g_z : g_wz;
    }
    if (a.g_foot_lever && lane < 4) {  // lane = leg (k = 0) holds its leg's sums
      double* o = a.g_foot_lever + (b * 4 + lane) * 3;
      o[0] = f0, o[1] = f1, o[2] = f2;
    }
  }
}

__global__ void __launch_bounds__(64) jvp_traj_kernel(int N, double dt, int64_t B, TrajJvpArgs a) {
  const int lane = threadIdx.x;
  const int k = lane >> 2, leg = lane & 3;
  const bool active = lane < 4 * N;
  const double tk = (double)(k + 1) * dt;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const TrajPoint q = traj_point(a.in, b, lane, N, dt);
    // the tangents of the per-robot scalars (uniform loads; a NULL array does not move)
    double dpx = 0.0, dpy = 0.0, dph = 0.0, dth = 0.0, dpsi = 0.0;
    if (a.d_x0) {
      const float* dx = a.d_x0 + b * 12;
      dpx = dx[0], dpy = dx[1], dph = dx[3], dth = dx[4], dpsi = dx[5];
    }
    double dvx = 0.0, dvy = 0.0, dz = 0.0, dwz = 0.0;
    if (a.d_cmd) {
      const float* dc = a.d_cmd + b * 4;
      dvx = dc[0], dvy = dc[1], dz = dc[2], dwz = dc[3];
    }
    const double dq0 = a.d_pos_des ? a.d_pos_des[b * 3] : 0.0;
    const double dq1 = a.d_pos_des ? a.d_pos_des[b * 3 + 1] : 0.0;
    const double dpdx = q.sx * dpx + (1.0 - q.sx) * dq0, dpdy = q.sy * dpy + (1.0 - q.sy) * dq1;
    const double dvwx = q.c * dvx - q.s * dvy - q.vwy * dpsi;
    const double dvwy = q.s * dvx + q.c * dvy + q.vwx * dpsi;
    if (a.d_pos_des_out && lane < 3)
      a.d_pos_des_out[b * 3 + lane] = lane == 0 ? dpdx : lane == 1 ? dpdy : dz;
    if (active) {
      const int64_t at = (b * N + k) * 12 + 3 * leg;
      if (a.d_xref) {  // columns 3 leg .. 3 leg + 2 of row k
        double v0 = 0.0, v1 = 0.0, v2 = 0.0;
        if (leg == 0) v0 = dpdx + dvwx * tk, v1 = dpdy + dvwy * tk, v2 = dz;
        if (leg == 1) v2 = dpsi + dwz * tk;
        if (leg == 2) v0 = dvwx, v1 = dvwy;
        if (leg == 3) v2 = dwz;
        float* o = a.d_xref + at;
        o[0] = (float)v0, o[1] = (float)v1, o[2] = (float)v2;
      }
      if (a.d_r_feet) {
        double r0 = 0.0, r1 = 0.0, r2 = 0.0;
        if (q.cls == kLeverCurrent && a.d_foot_lever) {
          const float* df = a.d_foot_lever + (b * 4 + leg) * 3;
          r0 = df[0], r1 = df[1], r2 = df[2];
        }
        if (q.cls >= 0) {
          const double dvbx = q.cth * dvx - q.sth * q.vxb * dth;
          const double dvby = (q.cth * q.sph * dth + q.sth * q.cph * dph) * q.vxb + q.sth * q.sph * dvx -
                              q.sph * q.vyb * dph + q.cph * dvy;
          const double dpj = dpsi + dwz * q.tj;
          const double dhwx = -q.hwy * dpj, dhwy = q.hwx * dpj;
          r0 = dhwx + q.tau * dvbx - q.tau * (dwz * q.hwy + q.wz * dhwy);
          r1 = dhwy + q.tau * dvby + q.tau * (dwz * q.hwx + q.wz * dhwx);
          r2 = -dz;
        }
        float* o = a.d_r_feet + at;
        o[0] = (float)r0, o[1] = (float)r1, o[2] = (float)r2;
      }
    }
  }
}

}  // namespace cmpc
