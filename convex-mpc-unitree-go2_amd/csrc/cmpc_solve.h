// cmpc_solve.h -- one QP instance: session control, the phases of solve_instance, the driver and
// the bin drain loop.
#pragma once
#include "cmpc_team.hip"  // W waves per QP for small batches (leader + helpers)

#include "cmpc_condense.h"
#include "cmpc_factor.h"
#include "cmpc_gradient.h"
#include "cmpc_polish.h"

namespace cmpc {

// ------------------------------------------------------------------------------------------
// one QP instance on one wave (W = 1) or led by wave 0 of a W-wave team (cmpc_team.hip)
// A polish session starts from the face set in s.code: record it as the session's first tried
// set and look it up among the starting sets of failed sessions.  Returns the session's repair
// budget (none for a remembered set).
template <int NC>
__device__ __forceinline__ int session_start(Smem<NC>& s, const KParams& P, int ntri, int nfail,
                                             int& ntried, bool& seen) {
  const int l = opaque_lane();
  WSYNC();
  uint8_t c = 0;
  if (l < ntri) {
    c = (uint8_t)s.code[l];
    s.tpat[0][l] = c;
  }
  ntried = 1;
  seen = false;
#pragma unroll
  for (int k = 0; k < kFailMem; ++k) {
    if (k >= nfail) break;  // uniform: only this instance's failed sessions
    const bool diff = (l < ntri) && (s.fpat[k][l] != c);
    seen |= (__any(diff) == 0);
  }
  if (seen) return 0;  // a remembered set is polished once more, without repairs
  // after two failed sessions the repair budget shrinks: a wandering repair sequence costs a
  // factorization per step (cfg1 +1 %, cfg2 +1-2 %)
  return (nfail >= 2) ? min(P.polish_repairs, kLateRepairs) : P.polish_repairs;
}

// Has the current session already tried the repaired face set in s.tcnt?
template <int NC>
__device__ __forceinline__ bool tried_before(Smem<NC>& s, int ntri, int ntried) {
  const int l = opaque_lane();
  WSYNC();
  const uint8_t c = (l < ntri) ? (uint8_t)s.tcnt[l] : 0;
  bool hit = false;
  for (int k = 0; k < ntried; ++k) {  // uniform trip count
    const bool diff = (l < ntri) && (s.tpat[k][l] != c);
    hit |= (__any(diff) == 0);
  }
  return hit;
}

// ------------------------------------------------------------------------------------------
// solve_instance and its phases.  The driver (solve_instance, at the end) stages the instance,
// picks the starting point and then loops: factorize when asked, one polish pass while a
// session is open (its outcome, a Polish value, selects the state changes), else one ADMM
// iteration, which may open a session.  The writers of w, y and lam follow the loop.
// ------------------------------------------------------------------------------------------

// Initial rho per bin: the NC >= 128 bins (33-64 stance triples) converge in fewer iterations
// from rho0 / 2; their hard instances (a failed polish session) go back to rho0, where they
// converge as before (NC = 128: cfg1 +6-10 %, cfg2 +1 %; NC >= 160: kRhoLowHeavy; rho0 / 2
// for the NC = 96 bin too loses 7 % on cfg2)
template <int NC>
constexpr bool kRhoLow = (NC == 128) || (kRhoLowHeavy && NC > 128);

// What the instance is: wave-uniform, fixed once stage_instance has run.
struct Instance {
  int64_t b;         // index in the batch
  int N, NP;         // horizon, 12 N
  Terrain T;         // this instance's mu / fz_min
  bool weights_ok;   // per-instance weights (Inputs::Q / R): valid?
  float r2_min;      // the strong-convexity modulus min_i R2[i] of this instance
  const float* Bg;   // its Bd [N][12][12]
  const float* xrb;  // its xref [N][12]
  int ntri, n;       // stance triples, ADMM params (3 ntri)
  bool nil;          // A = I + N, N^2 = 0: the closed-form condensation
  const f4* pwc;     // team mode, NC <= 128: the gradient's powers of A (else null)
  const f4* twc;
};

// What steers the solve loop: wave-uniform scalars, changed by the phases and by the driver's
// switch over a polish pass's outcome.
struct Ctl {
  int status = -2, iters = 0;
  bool polished = false;  // a polish pass accepted its point (the forces are in s.x)
  float rp = 0.f, rd = 0.f, np_ = 0.f, nd = 0.f;  // ADMM residuals and their scales
  float rho = 0.f;
  float inv_rho = 0.f;    // 1 / rho, divided out where rho is set (set_rho)
  bool rho_low = false;   // still at the bin's reduced initial rho
  int stable = 0;         // ADMM iterations since the face set last changed
  bool refactor = false;  // (re)build + invert the matrix for the current basis
  bool in_polish = false;
  int nact = 0;           // params of the current basis
  float shift = 0.f;      // sigma + rho (ADMM) or sigma (polish) on the matrix diagonal
  int it = 0;
  int it_adapt = 0;       // it % P.adaptive_interval and it % P.check_every, counted along with
  int it_check = 0;       // `it` (admm_iteration) instead of divided out every iteration
  int repairs_left = 0;
  int nadd = 0;           // faces added by downdates since the last factorization
  bool from_cand = false; // the polish refactored from a candidate that passed its check
  bool parked = false;    // the ADMM inverse is in the park slab
  int nfail = 0;          // failed sessions so far (the memory holds the last kFailMem)
  int ntried = 0;         // face sets tried in the current session
  bool seen_start = false;  // the current session started from a remembered failed set
  int last_pol = 0;       // iteration of the last polish session
  bool fail_rho_done = false;  // rho moved to kFailRho x rho0 after the first failed session
  bool warm_session = false;  // the current polish session is the warm start's
};

// ADMM goes on at `rho` (low: the bin's reduced initial rho): the matrix shift sigma + rho
// follows, and the matrix is factorized anew
__device__ __forceinline__ void set_rho(Ctl& c, const KParams& P, float rho, bool low) {
  c.rho = rho;
  c.inv_rho = uniformf(1.f / rho);
  c.rho_low = low;
  c.shift = uniformf(P.sigma + c.rho);
  c.refactor = true;
}

// Instance staging: global loads, validation and staging of Q / R, the stance triples, d_k, the
// ADMM basis and the nilpotent test.  Sets I's fields from weights_ok on (b, N, NP, T are the
// caller's).
template <int NC>
__device__ __forceinline__ void stage_instance(Smem<NC>& s, const KParams& P, const Inputs& in,
                                               Instance& I, int lane) {
  const int64_t b = I.b;
  const int N = I.N, NP = I.NP;
  const Terrain T = I.T;
  // per-instance weights (Inputs::Q / R): valid?  and the strong-convexity modulus min_i R2[i]
  // of this instance; both wave-uniform scalars like T, set with the staging loads below
  bool weights_ok = true;
  float r2_min = P.r2_min;
  const float* Ab = in.Ad + b * 144;
  const float* Bg = in.Bd + b * (int64_t)N * 144;
  const float* gdb = in.gd + b * 12;
  const float* x0b = in.x0 + b * 12;
  const float* xrb = in.xref + b * (int64_t)N * 12;
  const uint8_t* ctb = in.contact + b * (int64_t)4 * N;

  WSYNC();
  // First touch: everything the staging reads from global memory goes out in ONE round.  The
  // contact byte of (step, leg) = lane, and the instance's whole Bd as rows: lane l takes rows
  // 3 (l & 3) .. + 2 of step l >> 2, 36 consecutive floats (every byte of a fetched line is
  // used; the per-triple copy fetched 12-byte pieces 48 bytes apart, and only after the contact
  // scan had gone through the LDS).  build_admm_basis scatters the stance columns from these
  // registers once the scan is done; the tile registers are dead here, so they are free.
  const uint8_t ctv = (lane < 4 * N) ? ctb[(lane & 3) * N + (lane >> 2)] : (uint8_t)0;
  float bw[36];
  if (lane < 4 * N) {
    const float* src = Bg + lane * 36;
#pragma unroll
    for (int i = 0; i < 36; ++i) bw[i] = src[i];
  } else {
#pragma unroll
    for (int i = 0; i < 36; ++i) bw[i] = 0.f;
  }
  {  // one round of global loads: A, r_0..r_N (= x0, xref), gd; staged in LDS (G is free here)
    float av[3], rv[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int e = lane + 64 * i;
      av[i] = (e < 144) ? Ab[e] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = lane + 64 * i;
      rv[i] = (e < 12) ? x0b[e] : (e < 12 * (N + 1)) ? xrb[e - 12] : 0.f;
    }
    const float gv = (lane < 12) ? gdb[lane] : 0.f;
    // this instance's cost weights (Inputs::Q / R) over the wave's copies of the plan's
    // (drain_bin), which stay where the pointer is NULL.  Every reader of s.Q2 / s.R2 comes
    // after the WSYNC below; in team mode the helpers read them only inside a FACTOR command,
    // before that command's sweep barriers, which the leader passes with them: like s.A they
    // are rewritten here while the helpers wait at the next command's barrier.  An invalid row
    // (cmpc_plan_create's test of the constants; false also for NaN) takes the all-swing path
    // below, whose outputs depend on neither: finite stand-ins (Q2 = 0, R2 = 2) are stored.
    if (in.Q || in.R) {  // (uniform)
      const float q = (in.Q && lane < 12) ? in.Q[b * 12 + lane] : 0.f;
      const float r = (in.R && lane < 12) ? in.R[b * 12 + lane] : 1.f;
      weights_ok = __any(!(q >= 0.f && isfinite(q) && r > 0.f && isfinite(r))) == 0;
      if (lane < 12) {
        if (in.Q) s.Q2[lane] = weights_ok ? 2.f * q : 0.f;
        if (in.R) s.R2[lane] = weights_ok ? 2.f * r : 2.f;
      }
      if (in.R)
        r2_min = weights_ok ? uniformf(-wave_max((lane < 12) ? -2.f * r : -INFINITY)) : 2.f;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int e = lane + 64 * i;
      if (e < 144) s.A[e] = av[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) s.G[lane + 64 * i] = rv[i];
    if (lane < 12) s.G[256 + lane] = gv;
  }
  // stance triples in (k, leg) order; lane = 4k + leg.  An instance whose mu / fz_min entry or
  // Q / R row is invalid has no problem to solve: it takes the all-swing path (zero forces,
  // X = the rollout) and returns status -10
  const bool stc = lane < 4 * N && terrain_valid(T) && weights_ok && ctv != 0;
  const int pos = wave_excl_scan4(stc ? 1 : 0);
  const int ntri = wave_total4(stc ? 1 : 0);
  if (stc) s.tri[pos] = lane;
  if (lane < 4 * N) s.tri_of[lane] = stc ? pos : -1;
  WSYNC();
  {
    // d_k = A r_k + gd - r_{k+1}, r_0 = x0.  Entry o = 12 k + r, and a trip adds 64 = 5 x 12 + 4:
    // (k, r) are stepped along with o.  Row r of A and r_k are 16-byte aligned 12-float rows,
    // read as three f4 each; the sum runs over j ascending as before.
    static_assert(offsetof(Smem<NC>, A) % 16 == 0 && offsetof(Smem<NC>, G) % 16 == 0,
                  "the rows of A and r_k are read as f4");
    int k = lane / 12, r = lane - 12 * k;
    for (int o = lane; o < NP; o += 64) {
      const f4* ar = reinterpret_cast<const f4*>(&s.A[12 * r]);
      const f4* rk = reinterpret_cast<const f4*>(&s.G[12 * k]);
      float acc = s.G[256 + r] - s.G[12 * k + 12 + r];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const f4 av = ar[q], rv = rk[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = fmaf(av[j], rv[j], acc);
      }
      s.D[o] = acc;
      r += 4;
      k += 5;
      if (r >= 12) {
        r -= 12;
        ++k;
      }
    }
    build_admm_basis<NC>(s, P, Bg, ntri, &bw, __ballot(stc));
  }
  const bool nil = nilpotent_step(s);  // A = I + N, N^2 = 0: the closed-form condensation
  if (lane == 0) s.nil = nil ? 1 : 0;   // (and the gradient's powers of A)
  WSYNC();
  I.weights_ok = weights_ok;
  I.r2_min = r2_min;
  I.Bg = Bg;
  I.xrb = xrb;
  I.ntri = ntri;
  I.n = 3 * ntri;
  I.nil = nil;
}

// Starting point: x = z = y = 0 (cold), or the warm start from w_init, y_init or lam_init.
// s.pcode seeds the polish trigger (-1: no face set yet).
template <int NC>
__device__ __forceinline__ void starting_point(Smem<NC>& s, const Inputs& in, const Instance& I,
                                               float rho, int lane) {
  const int64_t b = I.b;
  const int N = I.N, NP = I.NP, n = I.n;
  const Terrain T = I.T;
  s.pcode[lane] = -1;
  if (in.w_init == nullptr && in.y_init == nullptr && in.lam_init == nullptr) {
    for (int p = lane; p < n; p += 64) { s.x[p] = 0.f; s.z[p] = 0.f; s.y[p] = 0.f; }
  } else if (lane < I.ntri) {
    // warm start (the reference's x0 / lam_x0 of centroidal_mpc.py:91-95): triple `lane`
    // (step k, leg l) starts at x = z = Pi_K(u_init), y = y_init; its face code seeds the
    // polish trigger with the projection of u + y / rho, the first z-update's argument
    const int kl = s.tri[lane];
    const int fo = 12 * (kl >> 2) + 3 * (kl & 3);
    float u[3] = {0.f, 0.f, 0.f}, yv[3] = {0.f, 0.f, 0.f};
    if (in.w_init) {
      const float* wi = in.w_init + b * (int64_t)(24 * N) + NP + fo;
#pragma unroll
      for (int a = 0; a < 3; ++a) u[a] = wi[a];
    }
    if (in.y_init) {
      const float* yi = in.y_init + b * (int64_t)NP + fo;
#pragma unroll
      for (int a = 0; a < 3; ++a) yv[a] = yi[a];
    } else if (in.lam_init) {
      // the reference's multipliers (centroidal_mpc.py:91-95 lam_x0 / lam_a0) -> this solver's
      // dual of the force: y = F' lam_fric + lam_x[u] (stationarity of the input rows:
      // 2R u - Bd' lam_eq + F' lam_fric + lam_x = 0 and y = -(2R u - Bd' lam_eq))
      const float* li = in.lam_init + b * (int64_t)(52 * N);
      const float* lf = li + 24 * N + NP + 16 * (kl >> 2) + 4 * (kl & 3);  // lam_a friction rows
      const float* lx = li + NP + fo;                                        // lam_x of the force
      const float f0 = lf[0], f1 = lf[1], f2 = lf[2], f3 = lf[3];
      yv[0] = f0 - f1 + lx[0];
      yv[1] = f2 - f3 + lx[1];
      yv[2] = -T.mu * (f0 + f1 + f2 + f3) + lx[2];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {  // non-finite warm data falls back to a cold start
      if (!isfinite(u[a])) u[a] = 0.f;
      if (!isfinite(yv[a])) yv[a] = 0.f;
    }
    float pv[3], qv[3];
    project(u[0], u[1], u[2], T.mu, T.fz_min, pv[0], pv[1], pv[2]);
    int code;
    if (in.y_init || in.lam_init) {  // the dual pushes the faces it holds outward (at the bin's initial rho)
      const float ir = 1.f / rho;
      code = project(pv[0] + yv[0] * ir, pv[1] + yv[1] * ir, pv[2] + yv[2] * ir, T.mu, T.fz_min,
                     qv[0], qv[1], qv[2]);
    } else {          // primal only: the faces the warm point lies on
      code = faces_at(pv[0], pv[1], pv[2], T.mu, T.fz_min, 1e-5f * pv[2]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s.x[3 * lane + a] = pv[a];
      s.z[3 * lane + a] = pv[a];
      s.y[3 * lane + a] = yv[a];
    }
    s.pcode[lane] = code;
  }
}

// Factorization: the only condense + invert call site.
template <int NC, int W>
__device__ __forceinline__ void factorize(Smem<NC>& s, const KParams& P, const Instance& I, Ctl& c,
                                          f4 (&M)[TeamCfg<NC, W>::SLOTS], TeamSmem<NC, W>* ts,
                                          int* seq, Diag& diag, int lane) {
  CMPC_CNT(8, 1);
  TRACEF(I.b, "it %d FACTOR polish %d nact %d shift %g\n", c.it, (int)c.in_polish, c.nact, c.shift);
  diag.factor();
  if constexpr (W == 1) {
    CMPC_T0(t_c);
    condense_tiles<NC>(s, P, M, c.nact, uniformf(c.shift), I.nil);
    CMPC_ACC(0, t_c);
    CMPC_T0(t_i);
    ldl_tiles<NC>(s, M, c.nact);
    CMPC_ACC(1, t_i);
  } else {
    CMPC_T0(t_c);
    team_factor_lead<NC, W>(s, *ts, *seq, P, M, c.nact, uniformf(c.shift));
    CMPC_ACC(0, t_c);
  }
  c.refactor = false;
}

// The factors of the last factorization applied to a param vector, out = (H + shift)^-1 in: the
// LDL' solve on this wave's register tiles (W = 1), or the team's symv with its explicit inverse
template <int NC, int W>
__device__ __forceinline__ void apply_factors(Smem<NC>& s, TeamSmem<NC, W>* ts, int* seq,
                                              const f4 (&M)[TeamCfg<NC, W>::SLOTS], int n,
                                              const float* in, float* out) {
  if constexpr (W == 1) ldl_apply<NC>(s, M, n, in, out);
  else team_symv_lead<NC, W>(s, *ts, *seq, M, n, in, out);
}

// The register tiles (factors or inverse) parked in the wave's global slab (W = 1), or each team
// wave's share in its part of the slab, the helpers by command
template <int NC, int W>
__device__ __forceinline__ void park_tiles(float* __restrict__ park, TeamSmem<NC, W>* ts, int* seq,
                                           const f4 (&M)[TeamCfg<NC, W>::SLOTS]) {
  if constexpr (W == 1) {
    park_store<NC>(park, M);
  } else {
    team_issue<NC, W>(*ts, *seq, kOpParkStore, 0, 0, 0);
    team_park_store<NC, W, 0>(park, M, 0);
  }
}

// The register tiles restored from where park_tiles left them
template <int NC, int W>
__device__ __forceinline__ void restore_tiles(const float* __restrict__ park, TeamSmem<NC, W>* ts,
                                              int* seq, f4 (&M)[TeamCfg<NC, W>::SLOTS]) {
  if constexpr (W == 1) {
    park_load<NC>(park, M);
  } else {
    team_issue<NC, W>(*ts, *seq, kOpParkLoad, 0, 0, 0);
    team_park_load<NC, W, 0>(park, M, 0);
  }
}

// A polish session opens on the face set in s.code: its repair budget and memory
// (session_start), the reduced basis (polish_setup from ADMM's z), and a factorization of it.
template <int NC>
__device__ __forceinline__ void enter_polish(Smem<NC>& s, const KParams& P, const Instance& I,
                                             Ctl& c) {
  c.repairs_left = session_start<NC>(s, P, I.ntri, c.nfail, c.ntried, c.seen_start);
  c.nact = polish_setup<NC>(s, P, I.T, I.Bg, I.ntri, s.z);
  c.nadd = 0;
  c.shift = P.sigma;
  c.refactor = true;
  c.in_polish = true;
}

// The current face set gets a fresh basis (polish_setup from the forces `from`) and a
// factorization; the downdates are gone.
template <int NC>
__device__ __forceinline__ void refactor_faces(Smem<NC>& s, const KParams& P, const Instance& I,
                                               Ctl& c, const float* from) {
  c.nact = polish_setup<NC>(s, P, I.T, I.Bg, I.ntri, from);
  c.nadd = 0;
  c.shift = P.sigma;
  c.refactor = true;
}

// What polish_refine leaves: the last refinement step, the scale of v, whether the steps
// stopped contracting, and the KKT check at the final point.
struct Refined {
  float step, vscale;
  bool stalled;
  PolishCheck chk;
};

// Iterative refinement v -= M (grad): polish_refine steps, then more (up to kRefineExtra)
// while the step still contracts and is above the acceptance tolerance -- an ill-conditioned
// face set (internal foot forces weigh only R) contracts slowly -- and then the KKT check.
template <int NC, int W>
__device__ __forceinline__ Refined polish_refine(Smem<NC>& s, const KParams& P, const Instance& I,
                                                 Ctl& c, f4 (&M)[TeamCfg<NC, W>::SLOTS],
                                                 TeamSmem<NC, W>* ts, int* seq, int lane) {
  Refined r;
  r.step = 3.0e38f;
  r.vscale = 1.f;
  r.stalled = false;
  float prev = 3.0e38f;
  const int nact = c.nact;
  // refinement steps before the convergence test may stop them: polish_refine from ADMM's
  // rough point; one from a candidate that already passed the check (a stall re-check)
  const int qmin = c.from_cand ? 1 : P.polish_refine;
  c.from_cand = false;
  for (int pass = 0;; ++pass) {
    // (an extra pass -- ambiguous face multipliers, below -- is one more refinement step)
    for (int q = pass == 0 ? 0 : P.polish_refine + kRefineExtra - 1;
         q < P.polish_refine + kRefineExtra; ++q) {
      gradient<NC, kGradLat<NC, W>, true>(s, P, nact, s.v, s.g, I.pwc, I.twc);
      apply_factors<NC, W>(s, ts, seq, M, nact, s.g, s.dl);
      if constexpr (W == 1) {  // (downdates: the one-wave kernels only, repair_faces)
        if (c.nadd > 0) dd_apply<NC>(s, nact, c.nadd, s.g, s.dl);  // (uniform)
      }
      float m = 0.f, mv = 1.f;
      for (int p = lane; p < nact; p += 64) {
        const float vn = s.v[p] - s.dl[p];
        s.v[p] = vn;
        m = fmaxf(m, fabsf(s.dl[p]));
        mv = fmaxf(mv, fabsf(vn));
      }
      r.step = wave_max(m);
      r.vscale = wave_max(mv);
      TRACEF(I.b, "    refine %d step %g\n", q, r.step);
      r.stalled = r.step > kRefineRate * prev;
      if (q + 1 >= qmin && (r.step <= P.polish_tol * wave_max(mv) || r.stalled)) break;
      prev = r.step;
    }
    gradient<NC, kGradLat<NC, W>, true>(s, P, nact, s.v, s.g, I.pwc, I.twc);  // E, L at the final point
    // a hard instance's later repairs move only the worst triples: full primal-dual
    // active-set steps swap several faces at a time and can wander between neighbouring sets
    const int top = (kRepairTop > 0 && (c.nfail > 0 || c.ntried >= 3)) ? kRepairTop : 0;
    r.chk = polish_check<NC>(s, P, I.T, I.Bg, I.ntri, r.step, top, trace_id(I.b));
    // A face multiplier near zero decides the check but moves by ~|H| x the point's remaining
    // error (a step accepted at polish_tol x the force scale leaves ~1e-5 N, i.e. ~1e-7 in a
    // multiplier -- the force-unit tolerance's size: config-3 instance 54289 passed with fz
    // held at fz_min, multiplier -3e-8 at its point, -1.3e-6 at the converged one, a
    // 1.2e-4 error; next-tick 55062 warm held fy at mu fz with +2.5e-7 at its point,
    // -3.2e-7 converged, 1.06e-4).  Such a check is repeated after further refinement steps.
    if (!(r.chk.amb && (r.chk.ok || r.chk.loose)) || pass >= kAmbRefine ||
        r.step <= kAmbConverged * P.polish_tol * r.vscale)
      break;
  }
  return r;
}

// What one polish pass decided; solve_instance's switch makes the state changes.
enum class Polish {
  kAccepted,         // the check passed: the forces are in s.x
  kAcceptedLoose,    // the session ends on a set within the loose tolerance (candidate in s.dl)
  kRefactorSameSet,  // a downdated refinement stalled: same faces, fresh factorization
  kRepaired,         // the check proposes a face set (s.tcnt) this session has not tried
  kWarmRestart,      // the warm start's session failed: restart as the cold solve
  kSessionFailed     // back to ADMM
};

// One polish pass: refinement, check, and exactly one decision.
template <int NC, int W>
__device__ __forceinline__ Polish polish_pass(Smem<NC>& s, const KParams& P, const Instance& I,
                                              const Outputs& out, Ctl& c,
                                              f4 (&M)[TeamCfg<NC, W>::SLOTS], TeamSmem<NC, W>* ts,
                                              int* seq, Diag& diag, int lane) {
  CMPC_T0(t_pol);
  Refined r = polish_refine<NC, W>(s, P, I, c, M, ts, seq, lane);
  const bool ok = r.chk.ok, loose = r.chk.loose;
  TRACEF(I.b, "it %d polish nact %d nadd %d ok %d loose %d changed %d amb %d dec %d step %g "
         "stalled %d repairs_left %d ntried %d nfail %d\n", c.it, c.nact, c.nadd, (int)ok,
         (int)loose, (int)r.chk.changed, (int)r.chk.amb, (int)r.chk.decisive, r.step,
         (int)r.stalled, c.repairs_left, c.ntried, c.nfail);
  CMPC_ACC(4, t_pol);
  // A refinement on a downdated inverse that stopped contracting above the tight level
  // (fp32 downdates of an ill-conditioned face set: steps 1e-4, 3.1e-5, 2.9e-5) leaves
  // multipliers near zero unreliable -- config-3 instance 31861 held a degenerate friction
  // face at -1.6e-7, released it, found it violated, and cycled through 5 sessions and 130
  // ADMM iterations.  When only such multipliers fail the check, the face set is refactored
  // exactly before the check decides.  (Refactoring every stalled downdate also fixed 31861
  // but cost 6-10 % more factorizations on configs 2-3: most stalls sit at the fp32 floor
  // of checks that large violations decide anyway.)
  // Nor is a point accepted while a downdated refinement stopped contracting above the
  // fp32 floor: the step is then no bound on the point's error (config-3 instance 39503:
  // three downdates, steps 2.2e-4, 5.7e-4, 5.0e-4 against a tolerance of 9.7e-4, accepted
  // 0.037 N = 3.8e-4 off; 25651: one downdate, steps 6.8e-5, 4.3e-5, 1.0e-4, 2.0e-4 off).
  // The face set is refactored and refined afresh first (round 6: the guard is the product
  // rule -- 9.5 % of config-3 instances, 18 % of config 2's, pass a check on such a
  // refinement, so answering them as status 2 instead was no option; profiles/r06a_*)
  const bool dd_stalled =
      c.nadd > 0 && r.stalled && r.step > kAmbConverged * P.polish_tol * r.vscale;
  const bool dd_stall = dd_stalled && (ok || loose || !r.chk.decisive);
  if (dd_stall) {
    r.chk.converged = false;
    if (out.stats != nullptr && lane == 0) atomicAdd(&out.stats[2], 1ull);  // (rare)
    diag.flag(Diag::kDdStall);
  }
  if (ok && !dd_stall) return Polish::kAccepted;
  if (c.nadd > 0 && !r.chk.converged) {
    // the downdated inverse stopped contracting: refactor the current face set, from the
    // candidate forces (not a repair)
    TRACEF(I.b, "it %d STALL-REFACTOR dd_stall %d\n", c.it, (int)dd_stall);
    c.from_cand = ok || loose;  // (the guard: the candidate passed; its error is what is checked)
    return Polish::kRefactorSameSet;
  }
  if (c.repairs_left > 0 && r.chk.changed && !tried_before<NC>(s, I.ntri, c.ntried))
    return Polish::kRepaired;
  if (loose) return Polish::kAcceptedLoose;
  return c.warm_session ? Polish::kWarmRestart : Polish::kSessionFailed;
}

// kAccepted.  Status 1 contract (include/cmpc.h): the check passed on a refinement that
// converged (and, after downdates, still contracted), and the held faces' certified force error
// is within kCertFace of the force scale (nilpotent step: the float64 rollout's multipliers); a
// point that misses the bound is returned as status 2
template <int NC>
__device__ __forceinline__ void accept_point(Smem<NC>& s, const Instance& I, const Outputs& out,
                                             Ctl& c, Diag& diag, int lane) {
  diag.accepted(s, I.r2_min, c.nact);
  const bool cert = !uniform(s.nil) || certified_faces<NC>(s, I.r2_min);
  if (!cert && out.stats != nullptr && lane == 0) atomicAdd(&out.stats[1], 1ull);
  if (!cert) diag.flag(Diag::kCertMiss);
  c.polished = true;
  c.status = cert ? 1 : 2;
}

// kAcceptedLoose: the candidate forces (s.dl) are the answer.
template <int NC>
__device__ __forceinline__ void accept_loose(Smem<NC>& s, const Instance& I, const Outputs& out,
                                             Ctl& c, Diag& diag, int lane) {
  diag.accepted(s, I.r2_min, c.nact);
  const bool certok = certified_faces<NC>(s, I.r2_min);
  const int l = opaque_lane();
  WSYNC();
  if (l < I.ntri) {  // (projected onto the pyramid: the loose check admits 5x polish_tol)
    float px, py, pz;
    project(s.dl[3 * l], s.dl[3 * l + 1], s.dl[3 * l + 2], I.T.mu, I.T.fz_min, px, py, pz);
    s.x[3 * l] = px;
    s.x[3 * l + 1] = py;
    s.x[3 * l + 2] = pz;
  }
  c.polished = true;
  // KKT-verified within the loose bounds only with the float64 rollout (polish_check) and
  // the certified face bound; a general A's loose acceptance is reported as not verified
  c.status = (uniform(s.nil) && certok) ? 1 : 2;
  if (out.stats != nullptr && lane == 0) {
    atomicAdd(&out.stats[0], 1ull);
    if (!certok) atomicAdd(&out.stats[1], 1ull);
  }
  diag.flag(Diag::kLoose | (certok ? 0 : Diag::kCertMiss));
}

// kRepaired: re-polish on the repaired face set (s.tcnt), on a downdated inverse where the
// repair only adds faces, else on a fresh factorization.
template <int NC, int W>
__device__ __forceinline__ void repair_faces(Smem<NC>& s, const KParams& P, const Instance& I,
                                             Ctl& c, f4 (&M)[TeamCfg<NC, W>::SLOTS], int lane) {
  const int ntri = I.ntri;
  --c.repairs_left;
  bool dd = false;
  if constexpr (W == 1) {
    // only added faces: downdate the inverse in the current basis (no refactorization)
    const int l = opaque_lane();
    WSYNC();
    const int oc = (l < ntri) ? s.code[l] : 0, nc = (l < ntri) ? s.tcnt[l] : 0;
    const int add = nc & ~oc;
    const int nf = wave_total4(face_count(add));
    if (trace_on(I.b)) {
      const bool drop = __any((nc & oc) != oc), freed = __any(((nc ^ oc) & oc & 1) != 0);
      TRACEF(I.b, "it %d repair drop %d (fz face freed %d) nf %d nadd %d cap %d\n", c.it,
             (int)drop, (int)freed, nf, c.nadd, dd_max(NC));
    }
    if (__any((nc & oc) != oc) == 0 && c.nadd + nf <= dd_max(NC)) {  // (uniform)
      CMPC_T0(t_dd);
      dd = face_downdate<NC>(s, I.T, M, c.nact, ntri, c.nadd);
      TRACEF(I.b, "it %d downdate nf %d -> %d nadd %d\n", c.it, nf, (int)dd, c.nadd);
      CMPC_ACC(28, t_dd);
      CMPC_CNT(29, 1);
      CMPC_CNT(30, nf);
    }
  }
  if (lane < ntri) {
    s.code[lane] = s.tcnt[lane];
    if (c.ntried < kTryMem) s.tpat[c.ntried][lane] = (uint8_t)s.tcnt[lane];
  }
  if (c.ntried < kTryMem) ++c.ntried;
  if (dd) return;  // refine on the downdated inverse
  refactor_faces<NC>(s, P, I, c, s.z);
}

// kWarmRestart.  The warm face set failed (the state moved across a face change): restart
// exactly as the cold solve of this problem -- x = z = y = 0, the bin's initial rho, no failed
// session on record -- so a warm start never takes more ADMM iterations than cold.
// (Continuing ADMM from the warm (x, z, y) counted the warm set as a failed session:
// 4 x rho0, 3x the stable run, the back-off -- the hard-instance schedule -- and the
// round-4 bench's warm maximum was 253 iterations against 107 cold.)
template <int NC>
__device__ __forceinline__ void warm_restart(Smem<NC>& s, const KParams& P, const Instance& I,
                                             Ctl& c) {
  c.warm_session = false;
  build_admm_basis<NC>(s, P, I.Bg, I.ntri);  // (zeroes x, z, y past n)
  {
    const int l = opaque_lane();
    for (int p = l; p < I.n; p += 64) { s.x[p] = 0.f; s.z[p] = 0.f; s.y[p] = 0.f; }
    s.pcode[l] = -1;
  }
  WSYNC();
  c.in_polish = false;
  c.nact = I.n;
  c.nadd = 0;
  set_rho(c, P, kRhoLow<NC> ? 0.5f * P.rho0 : P.rho0, kRhoLow<NC>);
  c.stable = 0;
  c.last_pol = 0;
  c.ntried = 0;
  c.seen_start = false;
  c.parked = false;
}

// kSessionFailed: remember the session's starting face set, restore the ADMM basis and go on
// with ADMM -- at another rho (c.refactor), on the parked inverse, or after a refactor.
template <int NC, int W>
__device__ __forceinline__ void session_failed(Smem<NC>& s, const KParams& P, const Instance& I,
                                               Ctl& c, f4 (&M)[TeamCfg<NC, W>::SLOTS],
                                               float* __restrict__ park, TeamSmem<NC, W>* ts,
                                               int* seq, Diag& diag, int lane) {
  c.warm_session = false;
  TRACEF(I.b, "it %d SESSION-FAIL nfail %d seen %d parked %d rho_low %d fail_rho_done %d nadd %d\n",
         c.it, c.nfail, (int)c.seen_start, (int)c.parked, (int)c.rho_low, (int)c.fail_rho_done,
         c.nadd);
  diag.session_failed();
  // the session failed: remember its starting face set (unless it came from the memory)
  if (!c.seen_start) {
    const int l = opaque_lane();
    if (l < I.ntri) s.fpat[c.nfail % kFailMem][l] = s.tpat[0][l];
    ++c.nfail;
  }
  // restore the basis and the parked ADMM inverse (or rebuild it first), continue ADMM
  build_admm_basis<NC>(s, P, I.Bg, I.ntri);
  c.in_polish = false;
  c.nact = I.n;
  if (c.nfail == 1 && !c.seen_start && kFailRho != 1.f && !c.fail_rho_done) {
    // the first failed session: a hard instance continues at kFailRho x rho0 (one refactor;
    // nothing is parked before the second session, so it would refactor anyway)
    c.fail_rho_done = true;
    set_rho(c, P, uniformf(kFailRho * P.rho0), false);
    return;
  }
  if (c.rho_low) {  // a hard instance: back to the standard rho0 (one refactor)
    set_rho(c, P, uniformf(P.rho0), false);
    return;
  }
  c.shift = uniformf(P.sigma + c.rho);
  if (c.parked) {
    restore_tiles<NC, W>(park, ts, seq, M);
  } else {
    c.refactor = true;  // M holds the polish inverse: refactor before the next iteration
  }
}

// One ADMM iteration, with the polish trigger and the rho adaptation.  Returns whether a polish
// session starts now.
template <int NC, int W>
__device__ __forceinline__ bool admm_iteration(Smem<NC>& s, const KParams& P, const Instance& I,
                                               Ctl& c, const f4 (&M)[TeamCfg<NC, W>::SLOTS],
                                               TeamSmem<NC, W>* ts, int* seq, int lane) {
  const int n = I.n, ntri = I.ntri, it = c.it;
  const Terrain T = I.T;
  const float alpha = P.alpha;
  float rho = c.rho;
  // the x-update's right-hand side r = rho (z - x) - g - y, entry by entry as the gradient's
  // closing loop forms g (its z, x and y reads go out with the loop's own)
  auto rhs = [&s, rho](int p, float gv, bool ok) {
    const float rp = rho * (s.z[p] - s.x[p]) - gv - s.y[p];
    if (ok) s.r[p] = rp;
  };
  gradient<NC, kGradLat<NC, W>, false, decltype(rhs)>(s, P, n, s.x, s.g, I.pwc, I.twc, rhs);
  apply_factors<NC, W>(s, ts, seq, M, n, s.r, s.dl);
  CMPC_T0(t_rest);
  const bool last = (it == P.max_iter);
  // (every iteration passes here once, right after the driver's ++c.it: the two counters wrap
  // where `it` reaches a multiple of their period)
  if (++c.it_adapt == P.adaptive_interval) c.it_adapt = 0;
  if (++c.it_check == P.check_every) c.it_check = 0;
  const bool adapt = P.adaptive_interval > 0 && c.it_adapt == 0;
  const float inv_rho = c.inv_rho;
  float lrp = 0.f, lrd = 0.f, lnp = 0.f, lnd = 0.f;
  bool changed = false;
  {
    const int l = opaque_lane();
    if (l < ntri) {
      float w[3], xr[3], xs[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int p = 3 * l + a;
        const float x = s.x[p], z = s.z[p];
        const float xt = x + s.dl[p];
        xr[a] = alpha * xt + (1.f - alpha) * z;
        xs[a] = alpha * xt + (1.f - alpha) * x;
        w[a] = xr[a] + s.y[p] * inv_rho;
      }
      float pv[3];
      const int code = project(w[0], w[1], w[2], T.mu, T.fz_min, pv[0], pv[1], pv[2]);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int p = 3 * l + a;
        const float zn = pv[a];
        const float yn = s.y[p] + rho * (xr[a] - zn);
        s.x[p] = xs[a];
        s.z[p] = zn;
        s.y[p] = yn;
        const float gp = s.g[p];
        lrp = fmaxf(lrp, fabsf(xs[a] - zn));
        lrd = fmaxf(lrd, fabsf(gp + yn));
        lnp = fmaxf(lnp, fmaxf(fabsf(xs[a]), fabsf(zn)));
        lnd = fmaxf(lnd, fmaxf(fabsf(gp), fabsf(yn)));
      }
      changed = code != s.pcode[l];
      s.pcode[l] = code;
      s.code[l] = code;
    }
  }
  if (trace_on(I.b)) {
    const float trp = wave_max(lrp), trd = wave_max(lrd);
    TRACEF(I.b, "it %d rho %g rp %g rd %g stable %d\n", it, rho, trp, trd, c.stable);
  }
  c.stable = (__any(changed) != 0) ? 0 : c.stable + 1;
  bool do_pol = false;
  // back off before a further attempt, longer after failed sessions: both the stable run and
  // the distance to the last session grow as polish_stable x 2^min(nfail, kBackoffCap)
  const int pstable = P.polish_stable;
  const int backoff = pstable << min(c.nfail, kBackoffCap);
  int need = pstable;  // (kStableGrow: the stable run required grows per failed session)
  for (int f = 0; f < min(c.nfail, kBackoffCap); ++f) need *= kStableGrow;
  if (c.stable >= need && !last && it - c.last_pol >= backoff &&
      (P.check_every == 1 || c.it_check == 0)) {  // (OPTS check_termination)
    do_pol = true;
    c.last_pol = it;
    c.stable = -backoff;
  }
  if (adapt || last) {
    c.rp = wave_max(lrp); c.rd = wave_max(lrd); c.np_ = wave_max(lnp); c.nd = wave_max(lnd);
  }
  if (adapt && !last) {
    float q = rho * sqrtf((c.rp / fmaxf(c.np_, 1e-30f)) / (c.rd / fmaxf(c.nd, 1e-30f) + 1e-30f));
    q = fminf(fmaxf(q, 1e-6f), 1e6f);
    if (q > 5.f * rho || q < 0.2f * rho) set_rho(c, P, uniformf(q), false);
  }
  CMPC_ACC(7, t_rest);
  return do_pol;
}

// Session start: parks the ADMM inverse when a failed session will need it back, then opens the
// session on ADMM's face set.
template <int NC, int W>
__device__ __forceinline__ void start_session(Smem<NC>& s, const KParams& P, const Instance& I,
                                              Ctl& c, const f4 (&M)[TeamCfg<NC, W>::SLOTS],
                                              float* __restrict__ park, TeamSmem<NC, W>* ts,
                                              int* seq, Diag& diag, int lane) {
  CMPC_CNT(9, 1);
  diag.polish_attempt();
  CMPC_T0(t_ps);
  // Park (write the 36-108 KB inverse to the wave's slab) only where a failed session will
  // restore it: not when a refactor is pending (rho changed: the inverse is stale), not at
  // the NC = 128 bin's reduced rho (a failure refactors at rho0), and not in the first
  // session (most instances pass it; the few that fail refactor once).  HBM writes of a
  // config-3 step drop from ~36 KB to a few hundred bytes per instance at unchanged speed.
  const bool pending = c.refactor;  // (trace)
  c.parked = !c.refactor && !c.rho_low && c.nfail > 0;
  if (c.parked) park_tiles<NC, W>(park, ts, seq, M);  // restored if the polish fails
  enter_polish<NC>(s, P, I, c);
  TRACEF(I.b, "it %d SESSION nfail %d parked %d rho %g refactor_pending %d seen %d repairs %d nact %d\n",
         c.it, c.nfail, (int)c.parked, c.rho, (int)pending, (int)c.seen_start, c.repairs_left,
         c.nact);
  CMPC_ACC(14, t_ps);
}

// Entry o of the force layout [k][leg][axis]: its axis a, and the stance triple of (k, leg) or -1
// on a swing leg
template <int NC>
__device__ __forceinline__ int force_triple(const Smem<NC>& s, int o, int& a) {
  const int k = o / 12, l = (o % 12) / 3;
  a = o % 3;
  return s.tri_of[4 * k + l];
}

// Output w: x_{k+1} = e_{k+1} + xref_k, u from the triples (zero on swing legs).  Returns
// whether every value written is finite.
template <int NC>
__device__ __forceinline__ bool write_w(Smem<NC>& s, const Instance& I, float* wb, bool polished,
                                        int lane) {
  const int NP = I.NP;
  const float* uf = polished ? s.x : s.z;  // polished forces overwrote x; else u = z
  int bad = 0;
  for (int o = lane; o < NP; o += 64) {
    const float xv = s.E[o] + I.xrb[o];
    int a;
    const int t = force_triple(s, o, a);
    const float uv = (t >= 0) ? uf[3 * t + a] : 0.f;
    bad |= !(isfinite(xv) && isfinite(uv));
    wb[o] = xv;
    wb[NP + o] = uv;
  }
  return __any(bad) == 0;
}

// Output y: the dual at the returned forces, in the force layout (zero on swing legs).
template <int NC, int W>
__device__ __forceinline__ void write_y(Smem<NC>& s, const KParams& P, const Instance& I,
                                        float* yb, bool polished, int lane) {
  const int NP = I.NP;
  if (polished && I.n > 0) {  // y = -grad f(u*) (the ADMM fixed point); s.g is the reduced one
    build_admm_basis<NC>(s, P, I.Bg, I.ntri);
    gradient<NC, kGradLat<NC, W>>(s, P, I.n, s.x, s.g, I.pwc, I.twc);
  }
  const float* yf = polished ? s.g : s.y;
  const float sg = polished ? -1.f : 1.f;
  for (int o = lane; o < NP; o += 64) {
    int a;
    const int t = force_triple(s, o, a);
    yb[o] = (t >= 0) ? sg * yf[3 * t + a] : 0.f;
  }
}

// Output lam: the reference's multipliers at the returned point (CasADi convention).
template <int NC>
__device__ __forceinline__ void write_lam(Smem<NC>& s, const Instance& I, float* lb, bool polished,
                                          int lane) {
  const int N = I.N, NP = I.NP;
  const Terrain T = I.T;
  if (!I.weights_ok) {  // an invalid Q / R row has no multipliers: a zero row
    for (int o = lane; o < 52 * N; o += 64) lb[o] = 0.f;
    return;
  }
  // L holds lambda_k = the adjoint at the returned forces (the last gradient call), and
  // lam_eq[k] = -lambda_k (stationarity of x_{k+1}).  Lane 4k + leg: s = 2R u + Bd_k' lambda_k
  // on its three forces, then the friction-row / bound multipliers of its faces.
  const float* uf = polished ? s.x : s.z;
  WSYNC();
  for (int o = lane; o < NP; o += 64) {
    lb[o] = 0.f;                 // lam_x of the states (free)
    lb[24 * N + o] = -s.L[o];    // lam_a of the dynamics rows
  }
  if (lane < 4 * N) {
    const int k = lane >> 2, leg = lane & 3;
    const int t = s.tri_of[lane];
    const float* Bk = I.Bg + k * 144 + 3 * leg;
    float sv[3], u[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      u[a] = (t >= 0) ? uf[3 * t + a] : 0.f;
      float acc = s.R2[3 * leg + a] * u[a];
#pragma unroll
      for (int r = 0; r < 12; ++r) acc = fmaf(Bk[r * 12 + a], s.L[12 * k + r], acc);
      sv[a] = acc;
    }
    float lf[4] = {0.f, 0.f, 0.f, 0.f}, lxv[3] = {0.f, 0.f, 0.f};
    if (t < 0) {  // swing: f = 0 by equal bounds, lam_x = -s
#pragma unroll
      for (int a = 0; a < 3; ++a) lxv[a] = -sv[a];
    } else {
      // (not polished: the faces the forces lie on)
      const int code = polished ? s.code[t]
                                : faces_at(u[0], u[1], u[2], T.mu, T.fz_min, 1e-5f * fmaxf(u[2], 1.f));
      // rows: fx - mu fz, -fx - mu fz, fy - mu fz, -fy - mu fz  (centroidal_mpc.py:332-355)
      if (code & 2) lf[0] = fmaxf(-sv[0], 0.f);
      if (code & 4) lf[1] = fmaxf(sv[0], 0.f);
      if (code & 8) lf[2] = fmaxf(-sv[1], 0.f);
      if (code & 16) lf[3] = fmaxf(sv[1], 0.f);
      if (code & 1) lxv[2] = fminf(-(sv[2] - T.mu * (lf[0] + lf[1] + lf[2] + lf[3])), 0.f);
    }
    float* lxo = lb + NP + 12 * k + 3 * leg;
#pragma unroll
    for (int a = 0; a < 3; ++a) lxo[a] = lxv[a];
    float* lfo = lb + 24 * N + NP + 16 * k + 4 * leg;
#pragma unroll
    for (int f = 0; f < 4; ++f) lfo[f] = lf[f];
  }
}

// The driver: one QP instance on this wave (W = 1) or led by it (W > 1).
template <int NC, int W>
__device__ __forceinline__ void solve_instance(Smem<NC>& s, const KParams& P, int64_t b,
                                               const Inputs& in, const Outputs& out,
                                               float* __restrict__ park, TeamSmem<NC, W>* ts,
                                               int* seq) {
  // W = 1: the whole lower triangle in this wave's registers; W > 1: this wave's team slots
  f4 M[TeamCfg<NC, W>::SLOTS];
  static_assert(W > 1 || TeamCfg<NC, W>::SLOTS == Cfg<NC>::NTL, "W = 1 holds every tile");
  const int lane = opaque_lane();
  Diag diag;
  Instance I;
  I.b = b;
  I.N = P.N;
  I.NP = 12 * P.N;
  I.T = instance_terrain(P, in, b);
  diag.poison(W == 1, s.G, 12 * NC, s.v, NC, park, Cfg<NC>::SLAB, lane);
  CMPC_T0(t_inst);
  CMPC_CNT(10, 1);
  stage_instance<NC>(s, P, in, I, lane);
  // team mode: the gradient's powers of A once per instance (registers to spare: the tiles are
  // split over the team)
  // (NC <= 128 only: the larger bins need those registers for their tiles)
  constexpr bool kPow = W > 1 && NC <= 128;
  f4 pw_c[4], tw_c[4];
  if constexpr (kPow) gradient_powers(s, pw_c, tw_c);
  I.pwc = kPow ? pw_c : nullptr;
  I.twc = kPow ? tw_c : nullptr;
  const int n = I.n;

  Ctl c;
  set_rho(c, P, kRhoLow<NC> ? 0.5f * P.rho0 : P.rho0, kRhoLow<NC>);
  starting_point<NC>(s, in, I, c.rho, lane);
  CMPC_ACC(6, t_inst);
  // ADMM state (x, z, y of triple t at 3t .. 3t+2) lives in LDS, not in registers
  diag.begin();
  c.refactor = n > 0;  // (no free force: nothing to factor)
  c.nact = n;
  if (n == 0) c.status = 1;
  if (n > 0 && in.w_init != nullptr) {
    // warm active set: the face set of the warm point goes straight to the polish (one
    // reduced factorization instead of the ADMM one + the polish one); if its KKT check and
    // repairs fail, the instance restarts as a cold solve (warm_restart)
    c.warm_session = true;
    WSYNC();
    if (lane < I.ntri) s.code[lane] = s.pcode[lane];
    enter_polish<NC>(s, P, I, c);
  }
  while (n > 0) {
    if (c.refactor) factorize<NC, W>(s, P, I, c, M, ts, seq, diag, lane);
    if (c.in_polish) {
      // (`continue`: round again, to factorize or to refine on a downdated inverse)
      switch (polish_pass<NC, W>(s, P, I, out, c, M, ts, seq, diag, lane)) {
        case Polish::kAccepted: accept_point<NC>(s, I, out, c, diag, lane); break;
        case Polish::kAcceptedLoose: accept_loose<NC>(s, I, out, c, diag, lane); break;
        case Polish::kRefactorSameSet: refactor_faces<NC>(s, P, I, c, s.dl); continue;
        case Polish::kRepaired: repair_faces<NC, W>(s, P, I, c, M, lane); continue;
        case Polish::kWarmRestart: warm_restart<NC>(s, P, I, c); continue;
        case Polish::kSessionFailed:
          session_failed<NC, W>(s, P, I, c, M, park, ts, seq, diag, lane);
          // only a session whose ADMM inverse came back from the park slab goes straight on
          if (c.refactor) continue;
          break;
      }
      if (c.polished) break;
    }
    if (c.it >= P.max_iter) break;
    c.iters = ++c.it;
    if (admm_iteration<NC, W>(s, P, I, c, M, ts, seq, lane))
      start_session<NC, W>(s, P, I, c, M, park, ts, seq, diag, lane);
  }
  if (!c.polished) {
    if (n > 0) {
      const bool conv = c.rp <= P.eps_abs + P.eps_rel * c.np_ && c.rd <= P.eps_abs + P.eps_rel * c.nd;
      c.status = conv ? 2 : -2;
    }
    gradient<NC, kGradLat<NC, W>>(s, P, n, s.z, s.g, I.pwc, I.twc);  // E at u = z (the pure rollout when every leg swings)
  }
  TRACEF(b, "END status %d iters %d\n", c.status, c.iters);
  CMPC_T0(t_out);
  WSYNC();
  float* wb = out.w + b * (int64_t)(24 * I.N);
  if (!write_w<NC>(s, I, wb, c.polished, lane) || !terrain_valid(I.T) || !I.weights_ok)
    c.status = -10;
  if (out.y) write_y<NC, W>(s, P, I, out.y + b * (int64_t)I.NP, c.polished, lane);
  if (out.lam) write_lam<NC>(s, I, out.lam + b * (int64_t)(52 * I.N), c.polished, lane);
  diag.finish(out.status, out.iters, wb, b, lane, c.status, c.iters);
  CMPC_CNT(11, c.iters);
  CMPC_ACC(15, t_out);
  CMPC_ACC(5, t_inst);
}

// Drain one bin's queue with this wave (persistent: instance ids come from a device counter).
// (W > 1: the leader's loop; the helpers leave their command loop at the closing kOpExit)
template <int NC, int W>
__device__ __forceinline__ void drain_bin(Smem<NC>& s, const KParams& P, const Inputs& in,
                                          const Outputs& out, const int* __restrict__ list,
                                          const int* __restrict__ count, int* __restrict__ head,
                                          float* __restrict__ park, TeamSmem<NC, W>* ts = nullptr,
                                          int* seq = nullptr) {
  const int lane = opaque_lane();
  WSYNC();
  // KParams copies (each bin's Smem layout places them differently); stage_instance overwrites
  // them per instance where Inputs::Q / R are given
  if (lane < 12) {
    s.Q2[lane] = P.Q2[lane];
    s.R2[lane] = P.R2[lane];
  }
  const int total = *count;
  for (;;) {
    int idx = 0;
    if (lane == 0) idx = atomicAdd(head, 1);
    idx = __builtin_amdgcn_readfirstlane(idx);
    if (idx >= total) break;
    const int64_t b = list[idx];
    solve_instance<NC, W>(s, P, b, in, out, park, ts, seq);
  }
  if constexpr (W > 1) team_issue<NC, W>(*ts, *seq, kOpExit, 0, 0, 0);
}

}  // namespace cmpc
