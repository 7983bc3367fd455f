// cmpc_instance.h -- geometry, tuning constants and the LDS image of one QP instance.
#pragma once
#include "cmpc_device.h"
#include "cmpc_wave_prims.h"

namespace cmpc {

// ------------------------------------------------------------------------------------------
// geometry and LDS image of one instance
// ------------------------------------------------------------------------------------------
constexpr int kMaxN = 16;
constexpr int kMaxP = 12 * kMaxN;   // 192
constexpr int kMaxTri = 4 * kMaxN;  // 64 = lanes: lane t owns stance triple t

template <int NC>
struct Cfg {
  static_assert(NC % 16 == 0, "bin capacity must be a multiple of 16");
  static constexpr int TT = NC / 16;             // 16x16 tile rows
  static constexpr int NTL = TT * (TT + 1) / 2;  // lower-triangle tiles (f4 per lane each)
  static constexpr int THREADS = 64;             // one wave per QP
  // per wave (floats): park slab of the register tiles (inverse or LDL' factors)
  static constexpr int SLAB = NTL * 256;
  // registers: the inverse (4 NTL) + working set; two waves per SIMD where it fits in 256
  static constexpr int WPE = (4 * NTL <= 150) ? 2 : 1;
};

// Polish sessions and their face sets.  A session starts from ADMM's face set and repairs it
// (primal-dual active-set steps, one factorization each).  Two memories cut the factorizations
// that hard instances used to spend on cycling:
//  * within a session, a repair that returns to a face set the session already tried ends the
//    session (the repair sequence has entered a cycle);
//  * a session that ends on a face set whose KKT violations are all within kLooseTol x the
//    polish tolerance is accepted: a weakly active face at a degenerate vertex can leave every
//    face set a few 1e-5 relative off in fp32 (the two sets of the cycle straddle it), and
//    5e-5 is still tighter than ADMM's own eps 1e-4 stop;
//  * the starting sets of the last kFailMem failed sessions are remembered; ADMM's face set can
//    stay "stable" while still wrong, and a session that starts from a remembered set polishes
//    it once more (it may pass now, from ADMM's better iterate) but makes no repairs.
constexpr int kRefineExtra = 4;      // polish refinements beyond polish_refine ...
constexpr float kRefineRate = 0.5f;  // ... while each step shrinks at least this much
constexpr int kBackoffCap = 3;       // polish back-off doubles per failed session, up to 8x
constexpr int kLateRepairs = 3;      // repair budget of the sessions after two failed ones
// Damped repairs (round 3).  A full primal-dual active-set step changes every violated triple
// at once; on the slow instances the polished point then violates a different handful of
// triples and the repairs wander between neighbouring face sets (traced on the NumPy model:
// 34087 made 16 repairs over four sessions, each changing 2-8 triples, maximum relative
// violation 0.02-1.0 throughout).  From the third repair of a session, and in every session
// after a failed one, a repair changes only the most violated half of the triples it would
// change (at least kRepairTop).  The first two repairs stay full steps, so an easy instance that
// misses its first polish is untouched.  A/B in one gpurun call, two alternations: the N = 8
// shard rehearsal 3.87 -> 2.99 ms, N = 4 5.18 -> 4.24 ms, config 2 at 8,192 3.72 -> 2.57 ms,
// config 3 at 8,192 +8 %, config 2 at 65,536 +2 %, config 3 at 65,536 and config 2 at 4,096
// unchanged; a fixed 2 (without the half) lost 35 % on config 2 at 4,096, a fixed 3 gained
// nothing on the shards.
constexpr int kRepairTop = 2;
// After each failed session (up to kBackoffCap) the face set must stay unchanged 3x longer
// before the next session: a hard instance's later sessions then start from a settled ADMM
// iterate instead of re-polishing a set that is still moving (ADMM iterations cost ~1/12 of a
// factorization).  NumPy model: slowest config-3 instance -21 %.  A/B in one gpurun call (two
// alternations, with the interior-point fallback off): N = 8 shard rehearsal 2.75 -> 2.43 ms,
// config 3 at 16,384 3.90 -> 3.65 ms, at 8,192 +3 %, at 65,536 +1 %, config 2 unchanged.
constexpr int kStableGrow = 3;
// The NC >= 160 bins also start at rho0 / 2 (round 3; NumPy model: -2.6 % cost in those bins).
// A/B in one gpurun call, two alternations: config 3 at 65,536 11.43 -> 11.26 ms, config 2 at
// 65,536 14.05 -> 13.67 ms, at 4,096 2.05 -> 1.95 ms, N = 8 shard rehearsal 2.51 -> 2.38 ms.
constexpr bool kRhoLowHeavy = true;
constexpr int kFailMem = 4;
constexpr int kTryMem = 8;
constexpr float kLooseTol = 5.f;
// Face multipliers in force units (polish_check, nilpotent step with the float64 rollout): a
// held face's multiplier must be >= -kFaceErr x polish_tol x us x R2 (a force error of at most
// ~5e-5 relative once released); a loose acceptance allows kLooseFace x that
constexpr float kFaceErr = 2.f;
constexpr float kLooseFace = 2.5f;
// status 1: the held faces' certified force error |c|_2 / min R2 (certified_faces) is at
// most this fraction of the force scale; with the check's primal tolerance (polish_tol, x5 for a
// loose acceptance, = 5e-5) the returned forces are within ~1e-4 of the optimum
constexpr float kCertFace = 5e-5f;
// A check decided by a face multiplier within polish_tol x gs of zero is repeated after up to
// kAmbRefine more refinement steps (unless the step is already below kAmbConverged x the
// acceptance tolerance)
constexpr int kAmbRefine = 2;
constexpr float kAmbBand = 5.f;
constexpr float kAmbConverged = 1e-2f;
// After its first failed polish session an instance continues ADMM at kFailRho x rho0.  The
// slow instances are the ones whose repairs cycle between neighbouring face sets (a degenerate
// corner of the pyramid: fz at fz_min with friction faces weakly active, coupled over steps);
// a stiffer rho settles ADMM's face set closer to the optimum's before the next session.  NumPy
// model (tests/algo_spec.py) over 8,192 config-3 / config-2 instances: mean factorizations
// unchanged, the slowest instance 30 -> 17 (config 3) and 42 -> 26 (config 2) factorizations.
constexpr float kFailRho = 4.f;

// Stride of a param's column in Smem::Bt.  (An odd stride, 13, spreads the gradient's per-step
// column reads over more LDS banks -- 12 puts the 16 steps' columns of a trot on 4 -- but it
// loses the 16-byte loads elsewhere: -1..-6 % on every workload, A/B in one gpurun call.)
constexpr int kBS = 12;

template <int NC>
struct Smem {
#ifdef CMPC_STAMPS
  unsigned long long st[32];       // per-wave stamp totals (flushed to g_stamps at exit)
#endif
  alignas(16) float Bt[NC * kBS];  // param-space input matrix, column p at Bt[kBS p .. kBS p + 11]
  alignas(16) float Rt[NC];        // param-space input weight (2R in the param basis)
  alignas(16) float x[NC];
  alignas(16) float z[NC];
  alignas(16) float y[NC];         // ADMM dual (x, z, y of triple t at 3t .. 3t+2)
  alignas(16) float v[NC];
  union {  // buffers that are dead while the matrix is condensed share the G slab
    struct {
      alignas(16) float g[NC];
      alignas(16) float r[NC];
      alignas(16) float dl[NC];
      alignas(16) float ds[NC];        // unit-diagonal scaling of the sweep
      alignas(16) float pan[NC * 4];   // sweep panel: 4 pivot columns, row-major [row][4]
      float H[kMaxP];                  // h_k = B~_k v_k + d~_k
      float E[kMaxP];                  // e_{k+1} = x_{k+1} - xref_k
      float L[kMaxP];                  // lambda_k
    };
    alignas(16) float G[NC * 12];      // condensation: G_t column p = A^{t-k_p} b_p
  };
  float D[kMaxP];                  // d_k  (error-coordinate affine term)
  float Dt[kMaxP];                 // d~_k (d_k + B_k t0_k in the polish basis)
  float A[144];
  float Q2[12];                    // KParams copies (indexed at run time -> keep out of kernarg),
                                   // or the instance's own 2Q / 2R (Inputs::Q / R, stage_instance)
  float R2[12];
  alignas(16) int par[NC];         // param -> step k
  int off[kMaxN + 1];              // first param of step k
  int nil;                         // A = I + N with N^2 = 0 (nilpotent_step): closed forms apply
  int tri[kMaxTri];                // stance triple t -> 4k + leg
  int tri_of[kMaxTri];             // 4k + leg -> triple index or -1
  int8_t tcnt[kMaxTri];            // polish: params of triple t / repaired face code
  int8_t code[kMaxTri];            // face code of triple t
  int8_t pcode[kMaxTri];           // face code of the previous ADMM iteration (-1: none)
  int fpk[kMaxTri];                // polish: params of triple t, px | py << 8 | pz << 16 (255 none)
  uint8_t fpat[kFailMem][kMaxTri]; // starting face sets of failed polish sessions
  uint8_t tpat[kTryMem][kMaxTri];  // face sets tried in the current session (0 = its start)
};

__device__ __forceinline__ constexpr int tile_index(int I, int J) { return (I * (I + 1)) / 2 + J; }

// One instance's friction coefficient and stance fz floor (Inputs::mu / fz_min, or the plan's
// constants).  The instance index is wave-uniform, so both are read through uniformf and live in
// scalar registers for the whole solve: no per-lane state (the solve kernels sit at the register
// ceiling).
struct Terrain {
  float mu, fz_min;
};
__device__ __forceinline__ Terrain instance_terrain(const KParams& P, const Inputs& in, int64_t b) {
  Terrain T{P.mu, P.fz_min};
  if (in.mu) T.mu = uniformf(in.mu[b]);
  if (in.fz_min) T.fz_min = uniformf(in.fz_min[b]);
  return T;
}
// (cmpc_plan_create's test of the plan's constants; false also for NaN)
__device__ __forceinline__ bool terrain_valid(const Terrain& T) {
  return T.mu > 0.f && isfinite(T.mu) && isfinite(T.fz_min);
}

// register tiles per wave and the park slab of a W-wave team (cmpc_team.hip; W = 1: the
// one-wave kernels)
template <int NC, int W>
struct TeamCfg {
  static constexpr int TT = NC / 16;
  static constexpr int NPAIR = TT / 2;
  static constexpr int PPW = (NPAIR + W - 1) / W;  // column pairs per wave
  // register tiles per wave (W = 1: the one-wave kernels, every lower tile)
  static constexpr int SLOTS = W == 1 ? TT * (TT + 1) / 2 : PPW * (TT + 1);
  static constexpr int SLAB = W * SLOTS * 256;     // park slab of the team (floats)
  static_assert(W == 1 || TT % 2 == 0, "team mode pairs tile columns");
};

}  // namespace cmpc
