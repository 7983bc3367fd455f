// cmpc_polish.h -- projection, the ADMM and polish bases, the KKT check and the face downdates.
#pragma once
#include "cmpc_factor.h"

namespace cmpc {

// Euclidean projection of (a, b, c) onto {|x| <= mu z, |y| <= mu z, z >= fz_min}.
// Face code bits: 1 fz at fz_min, 2/4 fx at +/-mu fz, 8/16 fy at +/-mu fz.
__device__ __forceinline__ int project(float a, float b, float c, float mu, float fzmin,
                                       float& px, float& py, float& pz) {
  const float Aa = fabsf(a), Bb = fabsf(b);
  const float lo = fminf(Aa, Bb), hi = fmaxf(Aa, Bb);
  const float z1 = (c + mu * (Aa + Bb)) / (1.f + 2.f * mu * mu);
  const float z2 = (c + mu * hi) / (1.f + mu * mu);
  float zz = (mu * z1 < lo) ? z1 : ((mu * z2 < hi) ? z2 : c);
  int code = 0;
  if (zz < fzmin) { zz = fzmin; code |= 1; }
  const float lim = mu * zz;
  if (a > lim) { px = lim; code |= 2; } else if (a < -lim) { px = -lim; code |= 4; } else px = a;
  if (b > lim) { py = lim; code |= 8; } else if (b < -lim) { py = -lim; code |= 16; } else py = b;
  pz = zz;
  return code;
}

// The faces a force on the pyramid lies on, to fp32 rounding (polish face code: 1 fz at fz_min,
// 2 / 4 fx at +/- mu fz, 8 / 16 fy alike).  `slack` is what the friction limit mu fz gives way
// by; the callers differ in it.
__device__ __forceinline__ int faces_at(float fx, float fy, float fz, float mu, float fz_min,
                                        float slack) {
  const float tz = 1e-5f * fmaxf(fz, 1.f), lim = mu * fz - slack;
  int code = (fz <= fz_min + tz) ? 1 : 0;
  code |= (fx >= lim) ? 2 : (fx <= -lim) ? 4 : 0;
  code |= (fy >= lim) ? 8 : (fy <= -lim) ? 16 : 0;
  return code;
}
// The faces among the bits `add` of a face code (one per axis at most)
__device__ __forceinline__ int face_count(int add) {
  return (add & 1) + ((add & 6) != 0) + ((add & 24) != 0);
}

// ADMM basis: every stance triple contributes (fx, fy, fz) as params 3t, 3t+1, 3t+2
template <int NC>
__device__ __forceinline__ void build_admm_basis(Smem<NC>& s, const KParams& P,
                                                 const float* __restrict__ Bg, int ntri,
                                                 const float (*bw)[36] = nullptr,
                                                 unsigned long long stance = 0) {
  const int lane = opaque_lane();
  const int N = P.N;
  const int n = 3 * ntri;
  WSYNC();
  if (bw != nullptr) {  // (a compile-time constant at every call site)
    // stage_instance's first-touch rows: lane l holds rows 3 (l & 3) .. + 2 of step l >> 2, all 12
    // columns.  It scatters the three columns of each stance leg of its step to that leg's
    // triple, whose index is the count of stance (step, leg) pairs before it in `stance`.
    const int k = lane >> 2, r0 = 3 * (lane & 3);
#pragma unroll
    for (int leg = 0; leg < 4; ++leg) {
      const int bit = 4 * k + leg;
      if ((stance >> bit) & 1ull) {
        const int t = __popcll(stance & ((1ull << bit) - 1ull));
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
          for (int rr = 0; rr < 3; ++rr) s.Bt[(3 * t + a) * kBS + r0 + rr] = (*bw)[rr * 12 + 3 * leg + a];
        }
      }
    }
  } else if (lane < ntri) {  // lane t copies the 12x3 block of its triple (all loads in flight at once)
    const int kl = s.tri[lane];
    const float* src = Bg + (kl >> 2) * 144 + 3 * (kl & 3);
    float bv[36];
#pragma unroll
    for (int r = 0; r < 12; ++r) {
#pragma unroll
      for (int a = 0; a < 3; ++a) bv[3 * r + a] = src[r * 12 + a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int r = 0; r < 12; ++r) s.Bt[(3 * lane + a) * kBS + r] = bv[3 * r + a];
    }
  }
  // param p = 3 t + a, and a trip adds 64 = 21 x 3 + 1: (t, a) are stepped along with p
  int t = lane / 3, a = lane - 3 * t;
  for (int p = lane; p < NC; p += 64, t += 21 + (a == 2), a = (a == 2) ? 0 : a + 1) {
    if (p < n) {
      const int kl = s.tri[t];
      s.Rt[p] = s.R2[3 * (kl & 3) + a];
      s.par[p] = kl >> 2;
    } else {
      s.Rt[p] = 0.f;
      s.par[p] = 0;
      s.x[p] = 0.f; s.z[p] = 0.f; s.g[p] = 0.f; s.r[p] = 0.f;
      s.v[p] = 0.f; s.dl[p] = 0.f;
    }
  }
  {  // off[k] = 3 x (stance (step, leg) pairs before step k): popcount of the stance mask
    const unsigned long long sm = __ballot(lane < 4 * N && s.tri_of[lane] >= 0);
    if (lane <= N) {
      const unsigned long long below = (lane >= 16) ? ~0ull : ((1ull << (4 * lane)) - 1ull);
      s.off[lane] = 3 * __popcll(sm & below);
    }
  }
  for (int o = lane; o < 12 * N; o += 64) s.Dt[o] = s.D[o];
  WSYNC();
}

// Polish setup: the reduced basis of the faces in s.code (lane t owns triple t),
// u = T v + t0 with t0 = locked components, v initialised from the triple forces in `vsrc`
// (ADMM's z, or the candidate forces a polish check left in s.dl; read before anything is
// written, since s.dl shares the G slab).  Returns nr; the param indices of each triple are
// left packed in s.fpk for the KKT check.
template <int NC>
__device__ __forceinline__ int polish_setup(Smem<NC>& s, const KParams& P, const Terrain& T,
                                            const float* __restrict__ Bg, int ntri,
                                            const float* vsrc) {
  const int lane = opaque_lane();
  const int N = P.N;
  const float mu = T.mu, fzmin = T.fz_min;
  WSYNC();
  const bool owns = lane < ntri;
  float vs[3] = {0.f, 0.f, 0.f};
  if (owns) {
#pragma unroll
    for (int a = 0; a < 3; ++a) vs[a] = vsrc[3 * lane + a];
  }
  WSYNC();
  const int code = owns ? s.code[lane] : 0;
  const int kl = owns ? s.tri[lane] : 0;
  const int k = kl >> 2, leg = kl & 3;
  const int sx = (code & 2) ? 1 : ((code & 4) ? -1 : 0);
  const int sy = (code & 8) ? 1 : ((code & 16) ? -1 : 0);
  const bool zl = (code & 1) != 0;
  const int cnt = owns ? ((sx == 0) + (sy == 0) + (!zl)) : 0;
  const int base = wave_excl_scan4(cnt);
  const int nr = wave_total4(cnt);
  if (owns) {
    float bx[12], by[12], bz[12];  // columns fx, fy, fz of B_k for this leg (loads in flight together)
    {
      const float* src = Bg + k * 144 + 3 * leg;
#pragma unroll
      for (int r = 0; r < 12; ++r) {
        bx[r] = src[r * 12];
        by[r] = src[r * 12 + 1];
        bz[r] = src[r * 12 + 2];
      }
    }
    s.tcnt[lane] = cnt;
    int p = base;
    int px = 255, py = 255, pz = 255;
    if (sx == 0) {
      px = p++;
#pragma unroll
      for (int r = 0; r < 12; ++r) s.Bt[px * kBS + r] = bx[r];
      s.Rt[px] = s.R2[3 * leg];
      s.par[px] = k;
      s.v[px] = vs[0];
    }
    if (sy == 0) {
      py = p++;
#pragma unroll
      for (int r = 0; r < 12; ++r) s.Bt[py * kBS + r] = by[r];
      s.Rt[py] = s.R2[3 * leg + 1];
      s.par[py] = k;
      s.v[py] = vs[1];
    }
    if (!zl) {
      pz = p++;
      const float cx = sx * mu, cy = sy * mu;
#pragma unroll
      for (int r = 0; r < 12; ++r) s.Bt[pz * kBS + r] = bz[r] + cx * bx[r] + cy * by[r];
      s.Rt[pz] = s.R2[3 * leg + 2] + mu * mu * ((sx != 0 ? s.R2[3 * leg] : 0.f) +
                                                (sy != 0 ? s.R2[3 * leg + 1] : 0.f));
      s.par[pz] = k;
      s.v[pz] = vs[2];
    } else {  // fz locked at fz_min: the triple's constant force t0 enters d~ through B_k t0
      const float tx = sx * mu * fzmin, ty = sy * mu * fzmin;
#pragma unroll
      for (int r = 0; r < 12; ++r) s.G[lane * 12 + r] = fmaf(bz[r], fzmin, fmaf(by[r], ty, bx[r] * tx));
    }
    s.fpk[lane] = px | (py << 8) | (pz << 16);
  }
  WSYNC();
  const unsigned long long sm = __ballot(lane < 4 * N && s.tri_of[lane] >= 0);
  {  // off[kk] = params of the triples before step kk = the scan base of the first triple of
     // step >= kk (its index: popcount of the stance mask below step kk), nr past the last
    const unsigned long long below = (lane >= 16) ? ~0ull : ((1ull << (4 * lane)) - 1ull);
    const int tstar = __popcll(sm & below);
    const int bt = __shfl(base, tstar < 64 ? tstar : 63, 64);
    if (lane <= N) s.off[lane] = (tstar < ntri) ? bt : nr;
  }
  {  // d~ = d + B t0 (LDS only).  Entry o = 12 kk + r, and a trip adds 64 = 5 x 12 + 4: (kk, r) are
     // stepped along with o.  The triple of (kk, leg) is the count of stance pairs before it in
     // the stance mask, and whether it locks fz is its bit of the wave's ballot of `zl`: what
     // s.tri_of and s.code hold, without their two dependent reads per leg.  The locked triples'
     // terms are added over the legs ascending as before.
    const unsigned long long zm = __ballot(zl);
    int kk = lane / 12, r = lane - 12 * kk;
    for (int o = lane; o < 12 * N; o += 64) {
      float acc = s.D[o];
      const unsigned m4 = (unsigned)(sm >> (4 * kk)) & 15u;
      int t = __popcll(sm & ((1ull << (4 * kk)) - 1ull));
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const bool st = ((m4 >> l) & 1u) != 0;
        if (st && ((zm >> t) & 1ull)) acc += s.G[t * 12 + r];
        t += st ? 1 : 0;
      }
      s.Dt[o] = acc;
      r += 4;
      kk += 5;
      if (r >= 12) {
        r -= 12;
        ++kk;
      }
    }
  }
  for (int p = lane; p < NC; p += 64)
    if (p >= nr) s.v[p] = 0.f;
  WSYNC();
  return nr;
}

// What polish_check found (all wave-uniform).
struct PolishCheck {
  bool ok;         // every KKT condition holds and the refinement step is within tolerance
  bool changed;    // the repaired face set (s.tcnt) differs from the checked one
  bool loose;      // every relative KKT violation (multipliers against the gradient scale, forces
                   // against the force scale) is within kLooseTol x polish_tol
  bool converged;  // the refinement step is within polish_tol x the force scale
  bool amb;        // a held face's multiplier lies within the ambiguity band of zero
  bool decisive;   // a violation outside that band fails the check
  float vworst;    // the largest relative violation
};

// Polish check after refinement (E, L at the final v in LDS): KKT conditions per triple
// (lane t = triple t, its params from s.fpk).  On success the triple's force is written over
// its ADMM primal s.x[3t .. 3t+2]; the repaired face code of a failing triple is left in
// s.tcnt and `changed` says whether any face changed.  For a loose acceptance the candidate
// forces are left in s.dl[3t .. 3t+2].
// top > 0: the repair changes only the `top` triples with the largest relative violation (the
// others keep their faces).  tr >= 0: trace the triples near a bound (cmpc_diag.h trace_id).
template <int NC>
__device__ __forceinline__ PolishCheck polish_check(Smem<NC>& s, const KParams& P,
                                                    const Terrain& T, const float* __restrict__ Bg,
                                                    int ntri, float step, int top = 0,
                                                    int tr = -1) {
  const int lane = opaque_lane();
  const float mu = T.mu, fzmin = T.fz_min;
  float fx = 0.f, fy = 0.f, fz = 0.f;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  bool lok = true;
  WSYNC();
  const bool owns = lane < ntri;
  const int code = owns ? s.code[lane] : 0;
  const int kl = owns ? s.tri[lane] : 0;
  const int k = kl >> 2, leg = kl & 3;
  const int sx = (code & 2) ? 1 : ((code & 4) ? -1 : 0);
  const int sy = (code & 8) ? 1 : ((code & 16) ? -1 : 0);
  const bool zl = (code & 1) != 0;
  if (owns) {
    // the forces on the current faces exactly (a face added by a downdate keeps its basis
    // param, which the refinement holds on the face only to rounding -- up to 1e-2 N off in
    // fp32 -- so the face's own value is taken, as for a face of the basis)
    const int pk = s.fpk[lane];
    const int px = pk & 255, py = (pk >> 8) & 255, pz = (pk >> 16) & 255;
    fz = zl ? fzmin : s.v[pz];
    fx = (sx == 0) ? s.v[px] : sx * mu * fz;
    fy = (sy == 0) ? s.v[py] : sy * mu * fz;
    const float* Bk = Bg + k * 144 + 3 * leg;
    float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll
    for (int r = 0; r < 12; ++r) {
      const float lr = s.L[12 * k + r];
      ax = fmaf(Bk[r * 12], lr, ax);
      ay = fmaf(Bk[r * 12 + 1], lr, ay);
      az = fmaf(Bk[r * 12 + 2], lr, az);
    }
    gx = ax + s.R2[3 * leg] * fx;
    gy = ay + s.R2[3 * leg + 1] * fy;
    gz = az + s.R2[3 * leg + 2] * fz;
  }
  const float gs = wave_max(fmaxf(fabsf(gx), fmaxf(fabsf(gy), fabsf(gz))));
  const float us = wave_max(fmaxf(1.f, fmaxf(fabsf(fx), fmaxf(fabsf(fy), fabsf(fz)))));
  const float tol_d = P.polish_tol * gs, tol_p = P.polish_tol * us;
  // Face multipliers.  A face held with multiplier -l moves the forces, once released, by up
  // to ~2.6 l / R2 (strong convexity: the condensed Hessian is >= diag(R2), and |a_f| <= 1.28
  // for a pyramid face), so with the float64 rollout (gradient<PREC>, nilpotent step) the
  // tolerance of each face is also bounded by kFaceErr x polish_tol x the force scale in those
  // units: 8e-8 at 200 N against ~5e-9 of gradient noise, where polish_tol x gs (the relative
  // test, ~5e-7) admitted 3458's -8.3e-7 (a 1.48e-4 error).  The general A keeps the fp32
  // rollout and the relative test.
  const bool prec = uniform(s.nil) != 0;
  float tfx = tol_d, tfy = tol_d, tfz = tol_d;
  if (prec && owns) {
    const float fe = kFaceErr * P.polish_tol * us;
    tfx = fminf(tol_d, fe * s.R2[3 * leg]);
    tfy = fminf(tol_d, fe * s.R2[3 * leg + 1]);
    tfz = fminf(tol_d, fe * s.R2[3 * leg + 2]);
  }
  bool ok = true, am = false, dec = false;
  int nc = 0;
  float v = 0.f, csq = 0.f;
  if (owns) {
    // KKT per triple; on a violation also derive the repaired face set (primal-dual
    // active-set step): drop faces with a negative multiplier, add violated faces
    const float lx = sx ? -sx * gx : 0.f;
    const float ly = sy ? -sy * gy : 0.f;
    const float l0 = gz - mu * (lx + ly);
    // (precise: a multiplier within kAmbBand x the relative band of zero is ambiguous at this
    // point -- the point's remaining error moves it by up to ~|H| x (step / 30))
    const float ta = kAmbBand * tol_d;
    am = prec && ((sx && lx < ta) || (sy && ly < ta) || (zl && l0 < ta));
    nc = code;
    if (sx && lx < -tfx) { ok = false; nc &= ~6; dec = dec || lx < -ta; }
    if (sy && ly < -tfy) { ok = false; nc &= ~24; dec = dec || ly < -ta; }
    if (zl && l0 < -tfz) { ok = false; nc &= ~1; dec = dec || l0 < -ta; }
    if (!sx && fabsf(fx) > mu * fz + tol_p) { ok = false; nc |= (fx > 0.f) ? 2 : 4; dec = true; }
    if (!sy && fabsf(fy) > mu * fz + tol_p) { ok = false; nc |= (fy > 0.f) ? 8 : 16; dec = true; }
    if (!zl && fz < fzmin - tol_p) { ok = false; nc |= 1; dec = true; }
    if (!(isfinite(fx) && isfinite(fy) && isfinite(fz))) { ok = false; dec = true; }
    const float ig = 1.f / fmaxf(gs, 1e-30f), iu = 1.f / us;
    v = fmaxf(fmaxf(sx ? -lx * ig : 0.f, sy ? -ly * ig : 0.f), zl ? -l0 * ig : 0.f);
    v = fmaxf(v, fmaxf(sx ? 0.f : (fabsf(fx) - mu * fz) * iu, sy ? 0.f : (fabsf(fy) - mu * fz) * iu));
    v = fmaxf(v, zl ? 0.f : (fzmin - fz) * iu);
    const bool fin = isfinite(fx) && isfinite(fy) && isfinite(fz);
    TRACE_IF(tr >= 0 && (v > 0.f || (sx && lx < tfx) || (sy && ly < tfy) || (zl && l0 < tfz)),
             "[%d]       tri %d k %d leg %d code %d f %g %g %g  l %g %g %g  tol %g %g %g  v %g\n",
             tr, lane, k, leg, code, fx, fy, fz, lx, ly, l0, tfx, tfy, tfz, v);
    lok = fin && v <= kLooseTol * P.polish_tol;
    // (precise: a loose acceptance also bounds the force error of every face it holds)
    if (prec)
      lok = lok && !(sx && lx < -kLooseFace * tfx) && !(sy && ly < -kLooseFace * tfy) &&
            !(zl && l0 < -kLooseFace * tfz);
    s.dl[3 * lane] = fx;  // the candidate, for a loose acceptance by the caller
    s.dl[3 * lane + 1] = fy;
    s.dl[3 * lane + 2] = fz;
    // certified force error of the held faces (status 1 contract): the point is the exact
    // optimum of the problem tilted by c = sum_f min(l_f, 0) a_f over the faces it holds
    // (a = (sx, 0, -mu), (0, sy, -mu), (0, 0, -1)), so |u - u*|_2 <= |c|_2 / min R2 (strong
    // convexity of the condensed objective, Hessian >= diag(R2))
    const float nx = sx ? fminf(lx, 0.f) : 0.f, ny = sy ? fminf(ly, 0.f) : 0.f;
    const float nz = zl ? fminf(l0, 0.f) : 0.f;
    const float cx = nx * sx, cy = ny * sy, cz = -mu * (nx + ny) - nz;
    csq = fmaf(cx, cx, fmaf(cy, cy, cz * cz));
    if (!isfinite(csq)) csq = INFINITY;
  }
  // (parked in the ADMM scratch s.r, which nothing reads before the next ADMM iteration or
  // face downdate rewrites it: certified_faces reduces it only for an accepted point)
  s.r[lane] = owns ? csq : 0.f;
  if (lane == 0) s.r[64] = us;
  if (top > 0) {  // uniform: keep the faces of all but the `top` most violated triples
    const bool cand = owns && nc != code;
    float key = cand ? (isfinite(v) ? v : INFINITY) : -1.f;  // a changed triple has v > 0
    bool sel = false;
    const int ncand = __popcll(__ballot(cand));
    const int kk = max(top, (ncand + 1) >> 1);  // (uniform)
    for (int r = 0; r < kk; ++r) {
      const float m = wave_max(key);
      if (!(m > 0.f)) break;  // uniform: no candidate left
      const unsigned long long bal = __ballot(key == m);
      if (lane == __builtin_ctzll(bal)) {
        sel = true;
        key = -1.f;
      }
    }
    if (cand && !sel) nc = code;
  }
  if (owns) s.tcnt[lane] = nc;  // repaired code (copied into s.code by the caller if used)
  PolishCheck res;
  res.changed = __any(owns && nc != code) != 0;
  res.amb = __any(am) != 0;
  // (only multipliers within the ambiguity band fail: the decision rests on the point's accuracy)
  res.decisive = __any(dec) != 0;
  res.vworst = wave_max((owns && isfinite(v)) ? v : (owns ? 1e30f : 0.f));
  const bool step_ok = step <= P.polish_tol * us;
  res.converged = step_ok;
  res.loose = (__all(lok) != 0) && step_ok;
  const bool all_ok = (__all(ok) != 0) && step_ok;
  res.ok = all_ok;
  if (all_ok && owns) {
    // onto the pyramid exactly: the check admits violations up to polish_tol x the force scale
    // (~2e-3 N), the reference's bounds take none (a move of at most that, far inside the 1e-4
    // parity bar)
    float px, py, pz;
    project(fx, fy, fz, mu, fzmin, px, py, pz);
    s.x[3 * lane] = px;
    s.x[3 * lane + 1] = py;
    s.x[3 * lane + 2] = pz;
  }
  return res;
}

// ------------------------------------------------------------------------------------------
// The certified force error of the held faces at the point polish_check accepted (its per-triple
// |c_t|^2 and the force scale are in s.r): within kCertFace of the force scale?  Uniform.
template <int NC>
__device__ __forceinline__ bool certified_faces(Smem<NC>& s, float r2_min) {
  const int lane = opaque_lane();
  WSYNC();
  const float c2 = wave_sum(s.r[lane]);
  return uniformf(sqrtf(c2)) <= kCertFace * r2_min * uniformf(s.r[64]);
}

// Face downdates (round 4).  A repair that only ADDS faces to the current face set keeps the
// basis and the inverse M of the last factorization: each added face is an equality a'v = c on
// the basis params (fz at fz_min: v_pz = fz_min; fx on the face of sign s: v_px - s mu v_pz = 0,
// or v_px = s mu fz_min where the basis locks fz; fy alike), and the inverse on the constrained
// set is the sequence of rank-1 downdates
//     M_j = M_{j-1} - w_j w_j' / d_j,   w_j = M_{j-1} a_j,   d_j = a_j' w_j,
// kept ASIDE: M stays in the register tiles untouched, the w_j are vectors in the polish
// session's free LDS (the sweep scaling / panel / H slab), and every refinement step applies
//     M_F g = M g - sum_j w_j (w_j' g) / d_j
// after its symv (dd_apply: one wave reduction per face).  w_j is one symv with the sparse a_j
// (two params at most) minus the earlier faces' terms, whose w_i' a_j are two LDS reads.  v is
// projected onto each new equality in the M_{j-1} metric, v -= w_j (a_j' v - c_j) / d_j, which
// keeps the earlier ones (a_i' w_j = 0, i < j).  Cost: a symv per added face instead of a
// condensation + inversion (~150 k cycles).  (Rank-4 MFMA updates of the tiles themselves do the
// same arithmetic, but writing the tiles in the polish branch kept them live across the KKT
// check and the register allocator spilled 600-1,100 VGPRs in every variant tried.)  NumPy model
// (tests/algo_spec.py downdate=True, the fp32 sweep inverse): unchanged refinement counts, half of
// all repairs are pure additions, and 6 faces per factorization keep almost all of the gain
// (config 3: 2.37 -> 2.19 factorizations per instance, the slowest instances -20 %).
// (diagnostic override only: -DCMPC_DD_CAP=3 exercises the refactor-on-cap path far more often;
// round 5 recorded its build as run-to-run non-deterministic, round 6's determinism records
// cover it)
#ifndef CMPC_DD_CAP
#define CMPC_DD_CAP 6
#endif
// faces per factorization: the w_j fill the ds / pan / H slab (5 NC + kMaxP floats) but its
// last 32 floats, which hold the faces' 1 / d_j, params, coefficients and right-hand sides
__host__ __device__ constexpr int dd_max(int NC) {
  return (5 * NC + kMaxP - 32) / NC < CMPC_DD_CAP ? (5 * NC + kMaxP - 32) / NC : CMPC_DD_CAP;
}
template <int NC>
__device__ __forceinline__ float* dd_w(Smem<NC>& s, int j) { return s.ds + j * NC; }
template <int NC>
__device__ __forceinline__ float* dd_meta(Smem<NC>& s) { return s.H + kMaxP - 32; }

// Append the faces added by the repair (s.code -> s.tcnt, no drops) as downdates; nadd counts
// the faces held so far.  False if they do not fit or a d_j is not positive (rounding after
// many downdates): the caller refactors.
template <int NC, class MT>
__device__ __forceinline__ bool face_downdate(Smem<NC>& s, const Terrain& T, const MT& M, int n,
                                              int ntri, int& nadd) {
  static_assert(dd_max(NC) >= 1 && dd_max(NC) <= 8, "the meta block holds 8 faces");
  static_assert(offsetof(Smem<NC>, H) == offsetof(Smem<NC>, ds) + 5 * NC * sizeof(float),
                "ds, pan and H are one slab");
  const int lane = opaque_lane();
  n = uniform(n);
  float* meta = dd_meta(s);  // [0, 8) 1 / d_j, [8, 16) p1 | p2 << 8, [16, 24) coefficient, [24, 32) c
  WSYNC();
  int F;
  {
    const bool owns = lane < ntri;
    const int oc = owns ? s.code[lane] : 0, nc = owns ? s.tcnt[lane] : 0;
    const int add = nc & ~oc;
    const int cnt = face_count(add);
    int j = nadd + wave_excl_scan4(cnt);
    F = uniform(wave_total4(cnt));
    if (nadd + F > dd_max(NC)) return false;  // (uniform)
    if (owns && add) {
      // a face with no second param has p2 = p1 and coefficient 0
      // (fz_min's vector copy is made here: hoisted to the instance loop's head it stayed live
      // for the whole solve and was one more spilled register of the NC 128 kernel)
      const float mu = T.mu;
      float fzmin = T.fz_min;
      asm volatile("" : "+v"(fzmin));
      const int pk = s.fpk[lane];
      const int px = pk & 255, py = (pk >> 8) & 255, pz = (pk >> 16) & 255;
      if (add & 1) {  // (first: a friction face added with it then reads fz = fz_min)
        meta[8 + j] = __int_as_float(pz | (pz << 8)); meta[16 + j] = 0.f; meta[24 + j] = fzmin; ++j;
      }
#pragma unroll
      for (int ax = 0; ax < 2; ++ax) {
        const int bits = ax ? (add & 24) : (add & 6);
        if (!bits) continue;
        const int pa = ax ? py : px;
        const float sg = (bits & (ax ? 8 : 2)) ? 1.f : -1.f;
        if (pz != 255) {
          meta[8 + j] = __int_as_float(pa | (pz << 8)); meta[16 + j] = -sg * mu; meta[24 + j] = 0.f;
        } else {
          meta[8 + j] = __int_as_float(pa | (pa << 8)); meta[16 + j] = 0.f; meta[24 + j] = sg * mu * fzmin;
        }
        ++j;
      }
    }
  }
  WSYNC();
  const int j1 = nadd + F;
  for (int j = nadd; j < j1; ++j) {  // uniform
    const int q = __float_as_int(meta[8 + j]);
    const int p1 = q & 255, p2 = (q >> 8) & 255;
    const float cf = meta[16 + j], cv = meta[24 + j];
    for (int p = lane; p < NC; p += 64) s.r[p] = (p == p1) ? 1.f : (p == p2) ? cf : 0.f;
    float* w = dd_w(s, j);
    ldl_apply<NC>(s, M, n, s.r, w);  // w = M a_j
    for (int i = 0; i < j; ++i) {  // w -= w_i (w_i' a_j) / d_i  (uniform trip count)
      const float* wi = dd_w(s, i);
      const float t = fmaf(cf, wi[p2], wi[p1]) * meta[i];
      for (int p = lane; p < n; p += 64) w[p] = fmaf(-t, wi[p], w[p]);
      WSYNC();
    }
    const float d = fmaf(cf, w[p2], w[p1]);
    if (!(d > 0.f) || !isfinite(d)) return false;  // (the same value in every lane)
    const float id = 1.f / d;
    const float res = (fmaf(cf, s.v[p2], s.v[p1]) - cv) * id;
    WSYNC();
    for (int p = lane; p < n; p += 64) s.v[p] = fmaf(-res, w[p], s.v[p]);  // v onto a_j' v = c_j
    if (lane == 0) meta[j] = id;
    WSYNC();
  }
  nadd = j1;
  return true;
}

// dl = M_F g from dl = M g: dl -= sum_j w_j (w_j' g) / d_j over the nadd faces held
template <int NC>
__device__ __forceinline__ void dd_apply(Smem<NC>& s, int n, int nadd, const float* gin,
                                         float* dl) {
  const int lane = opaque_lane();
  const float* meta = dd_meta(s);
  n = uniform(n);
  WSYNC();
  float sj[dd_max(NC)];
#pragma unroll
  for (int j = 0; j < dd_max(NC); ++j) {
    if (j >= nadd) break;  // uniform
    const float* w = dd_w(s, j);
    float part = 0.f;
    for (int p = lane; p < n; p += 64) part = fmaf(w[p], gin[p], part);
    sj[j] = wave_sum(part) * meta[j];
  }
  for (int p = lane; p < n; p += 64) {
    float acc = dl[p];
#pragma unroll
    for (int j = 0; j < dd_max(NC); ++j) {
      if (j >= nadd) break;
      acc = fmaf(-sj[j], dd_w(s, j)[p], acc);
    }
    dl[p] = acc;
  }
  WSYNC();
}

}  // namespace cmpc
