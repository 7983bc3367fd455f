/*
 * cmpc.h -- C-ABI of the MI355X batched convex-MPC contact-force QP solver.
 *
 * Drop-in boundary for the QP solve of ltinphan/convex-mpc-unitree-go2:
 *   convex_mpc/centroidal_mpc.py:212-213  ca.conic('S', 'osqp', {h, a}, OPTS)   -> cmpc_plan_create
 *   convex_mpc/centroidal_mpc.py:76-98    _update_sparse_matrix + _compute_bounds
 *                                         + self.solver(h, g, a, lba, uba, lbx, ubx)
 *                                                                                -> cmpc_solve
 *   convex_mpc/centroidal_mpc.py:113-119  self.solver.stats()['return_status']  -> status[]
 *
 * One call solves B independent instances of the reference QP (centroidal_mpc.py:122-359):
 *   min  sum_k (x_{k+1}-xref_k)' Q (x_{k+1}-xref_k) + u_k' R u_k
 *   s.t. x_{k+1} = Ad x_k + Bd_k u_k + gd           (k = 0..N-1, x_0 given)
 *        swing leg:  f = 0                           (centroidal_mpc.py:150-161)
 *        stance leg: fz >= fz_min, |fx| <= mu fz, |fy| <= mu fz
 *                                                    (centroidal_mpc.py:163-170, 264-283, 324-359)
 * which is exactly ½w'Hw + g'w of the reference with H = diag(2Q.., 2R..), g = [-2Q xref; 0]
 * (up to the constant sum xref'Q xref).
 *
 * Layouts (row-major, all device pointers, caller-owned):
 *   Ad      [B][12][12]        fp32   (traj.Ad)
 *   Bd      [B][N][12][12]     fp32   (traj.Bd)
 *   gd      [B][12]            fp32   (traj.gd)
 *   x0      [B][12]            fp32   (traj.initial_x_vec)
 *   xref    [B][N][12]         fp32   (traj.compute_x_ref_vec() transposed: xref[b][k] is the
 *                                      reference's column k = target for x_{k+1})
 *   contact [B][4][N]          uint8  (traj.contact_table, legs FL FR RL RR; nonzero = stance)
 *   w_out   [B][24N]           fp32   reference decision layout (centroidal_mpc.py:44,
 *                                      test_MPC.py:190-192): w = [x_1..x_N | u_0..u_{N-1}],
 *                                      each 12 contiguous, i.e. vec(X (12,N),'F') then vec(U,'F')
 *   status  [B]                int32  1 solved: an active-set polish passed the KKT check --
 *                                       primal violations <= polish_tol x the force scale us
 *                                       (<= 5 x for a loose acceptance; the returned forces are
 *                                       then projected onto the pyramid), a refinement step
 *                                       <= polish_tol x us that was still contracting (never
 *                                       one stalled on a face-downdated factorization), and, for
 *                                       the reference's nilpotent step matrix (float64 rollout),
 *                                       a CERTIFIED bound on the force error of the held faces:
 *                                       with c = sum_f min(lambda_f, 0) a_f over the faces held,
 *                                       |u - u*|_2 <= |c|_2 / min(2R) <= 5e-5 x us (strong
 *                                       convexity).  Together: within ~1e-4 of the optimum
 *                                       except along directions weighed only by R, which the
 *                                       fp32 refinement resolves poorly (fresh-seed surveys:
 *                                       2 of 196,606 status-1 answers at 1.1e-4 / 2.1e-4 at
 *                                       polish_refine 2, none above 5.6e-5 at polish_refine 4,
 *                                       DESIGN.md 8).
 *                                     2 solved inaccurate: ADMM residuals within eps, or a polished
 *                                       point that misses the certified bound (returned, but not
 *                                       verified to 1e-4),
 *                                     -2 max iterations.
 *                                       There is no residual-based early stop: an instance ends
 *                                       through a polish or at max_iter, so status 2 can only be
 *                                       returned at iters == max_iter or for a polished point
 *                                       that misses the bound.  At max_iter without an accepted
 *                                       polish the forces returned are ADMM's z, and the status
 *                                       is 2 when rp <= eps_abs + eps_rel np and
 *                                       rd <= eps_abs + eps_rel nd, else -2, on the last
 *                                       iteration's values of (infinity norms over the stance
 *                                       forces; x, z, y after that iteration's updates, g the
 *                                       gradient P x + q of the condensed cost at the x the
 *                                       iteration started from)
 *                                         rp = |x - z|,  np = max(|x|, |z|),
 *                                         rd = |g + y|,  nd = max(|g|, |y|).
 *                                       These are this solver's definitions, not OSQP's (whose
 *                                       dual scale is max(|P x|, |q|, |y|)).
 *                                     -10 numerical failure or an invalid
 *                                       per-instance mu / fz_min entry or Q / R row
 *                                       (cmpc_solve_io)
 *   iters   [B]                int32  ADMM iterations taken
 *
 * Threading: one plan per host thread / stream.  cmpc_solve is asynchronous on `stream`
 * (a hipStream_t, NULL = default stream); it performs no allocation, no host synchronisation
 * and is graph-capturable.  Return codes are 0 or a negative CMPC_E* value; the message is
 * available from cmpc_last_error() (thread-local).
 */
#ifndef CMPC_H_
#define CMPC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 6: status 1 carries a certified force-error bound (see status above); cmpc_plan_stats.
 * 5: the interior-point variant and its cmpc_plan_set_ipm / cmpc_plan_ipm_batch are gone
 *    (cmpc_params.reserved0 must be 0).  4: three solve-kernel timing slots. */
#define CMPC_ABI_VERSION 6

#define CMPC_OK 0
#define CMPC_E_INVALID (-22)   /* bad argument / parameter (EINVAL) */
#define CMPC_E_NOMEM (-12)     /* device allocation failed (ENOMEM) */
#define CMPC_E_HIP (-5)        /* HIP runtime error (EIO) */
#define CMPC_E_RANGE (-34)     /* batch larger than the plan's max_batch (ERANGE) */

/* Solver parameters.  cmpc_params_default() fills the reference's values
 * (centroidal_mpc.py:12-38, fz_min from :127) and this solver's ADMM settings. */
typedef struct cmpc_params {
  int32_t abi_version;    /* must be CMPC_ABI_VERSION */
  int32_t N;              /* horizon, 1..16 (reference: 16, com_trajectory.py:66) */
  float Q[12];            /* state weight diagonal (centroidal_mpc.py:12) */
  float R[12];            /* input weight diagonal (centroidal_mpc.py:13) */
  float mu;               /* friction coefficient (centroidal_mpc.py:15) */
  float fz_min;           /* stance normal-force lower bound (centroidal_mpc.py:127) */
  float eps_abs;          /* ADMM residual tolerances for status 2 (OPTS eps_abs/eps_rel), both
                             finite and >= 0; the test is stated under `status` above */
  float eps_rel;
  int32_t max_iter;       /* ADMM iteration cap (OPTS max_iter) */
  float rho;              /* initial ADMM penalty (the bins with more than 96 free forces start
                             at rho / 2 and return to rho after a failed polish session; a free
                             force is one axis of a stance (step, leg) pair) */
  float sigma;            /* ADMM proximal regularisation (OSQP sigma) */
  float alpha;            /* over-relaxation (OSQP alpha) */
  int32_t adaptive_rho_interval; /* iterations between rho updates (0 = off).  At an iteration
                             that is a multiple of it and not the last (iteration < max_iter),
                             with rp, rd, np, nd of that iteration as defined under `status`:
                             rho' = clip(rho sqrt((rp / np) / (rd / nd)), 1e-6, 1e6), taken (and
                             the matrix factorized anew) when rho' > 5 rho or rho' < rho / 5 */
  int32_t polish_stable;  /* polish after the active set is unchanged this many iterations */
  int32_t polish_refine;  /* refinement steps inside the polish before its convergence test may
                             stop them (up to 4 more while the step still halves); default 2
                             (4: ~5 % slower, tighter along R-weighted directions) */
  float polish_tol;       /* relative KKT tolerance for accepting the polished point */
  int32_t polish_repairs; /* active-set repairs (add violated / drop negative-multiplier faces
                             and re-polish) before resuming ADMM */
  int32_t reserved0;      /* must be 0 (ABI 4's ipm_facts: the interior-point fallback was
                             removed in ABI 5) */
  int32_t check_termination; /* ADMM iterations between termination tests (OPTS check_termination,
                             centroidal_mpc.py:31): the polish trigger (face set stable for
                             polish_stable iterations -> active-set polish + KKT check, the only
                             way an instance ends solved) is evaluated only at iterations that
                             are multiples of it.  Default 1: here the test is one wave ballot
                             of the face codes, so checking every iteration costs nothing, while
                             OSQP's 10 amortises a residual evaluation (two sparse matvecs) this
                             solver does not need.  The reference's 10 is accepted (the drop-in
                             CentroidalMPC passes it): same solutions, iterations rounded up to
                             multiples of 10. */
  int64_t max_batch;      /* largest B passed to cmpc_solve (sizes plan workspace) */
} cmpc_params;

typedef struct cmpc_plan cmpc_plan;

/* Fill *p with defaults.  Replaces the OPTS dict (centroidal_mpc.py:20-36). */
void cmpc_params_default(cmpc_params* p);

/* Validate params, allocate workspace for max_batch instances on the current device.  Every
 * later call with this plan must run with that device current (else CMPC_E_INVALID).
 * Replaces CentroidalMPC.__init__/_build_sparse_matrix (centroidal_mpc.py:41-67,178-230). */
int cmpc_plan_create(const cmpc_params* p, cmpc_plan** out);

/* Solve B instances (see layouts above).  Replaces CentroidalMPC.solve_QP's update + solve
 * (centroidal_mpc.py:69-120) for a whole batch.  `stream` is a hipStream_t or NULL. */
int cmpc_solve(cmpc_plan* plan, int64_t B, const float* Ad, const float* Bd, const float* gd,
               const float* x0, const float* xref, const uint8_t* contact, float* w_out,
               int32_t* status, int32_t* iters, void* stream);

/* Warm-started solve: the reference's x0 / lam_x0 / lam_a0 warm start
 * (centroidal_mpc.py:91-95, kept from the previous solve at :108-110; OPTS warm_start_primal /
 * warm_start_dual, :33-34).  As cmpc_solve, plus:
 *   w_init  [B][24N]  fp32  nullable; a previous w_out (optionally shifted by the caller).
 *                           Only the force part (w_init[b][12N + 12k + 3l + a]) is used: each
 *                           stance force starts at its projection onto the friction pyramid.
 *   y_init  [B][12N]  fp32  nullable; a previous y_out (force layout, swing entries ignored).
 *   y_out   [B][12N]  fp32  nullable; this solver's dual at the returned forces: -grad of the
 *                           condensed objective at u* (zero on swing legs).  It is cmpc's own
 *                           multiplier, not OSQP's lam_a (there are no constraint rows here).
 * With w_init, the faces of the friction pyramid the warm point holds (its forces on a face to
 * fp32 rounding, or pushed outward by y_init) go straight to the active-set polish: when that
 * face set (after up to polish_repairs repairs) passes the KKT check, the solve takes one
 * reduced factorization and no ADMM iteration (iters = 0).  Otherwise ADMM starts from
 * x = z = the projected warm forces, y = y_init (or 0).
 * NaN/Inf warm entries start at zero.  w_init may alias w_out and y_init may alias y_out (every
 * instance reads its warm data before it writes its outputs).  Both NULL == cmpc_solve. */
int cmpc_solve_warm(cmpc_plan* plan, int64_t B, const float* Ad, const float* Bd,
                    const float* gd, const float* x0, const float* xref,
                    const uint8_t* contact, const float* w_init, const float* y_init,
                    float* w_out, float* y_out, int32_t* status, int32_t* iters, void* stream);

/* Solve with the REFERENCE's multipliers (SURVEY.md 8(b) y_inout; centroidal_mpc.py:91-95
 * warm start lam_x0 / lam_a0, :108-110 sol["lam_x"] / sol["lam_a"]).  As cmpc_solve, plus:
 *   w_init    [B][24N]  fp32  nullable; primal warm start, as for cmpc_solve_warm.
 *   lam_init  [B][52N]  fp32  nullable; warm duals in the reference layout
 *                             [lam_x (24N: states, then forces) | lam_a (28N: 12N dynamics rows,
 *                             then 16N friction rows fx-mu fz, -fx-mu fz, fy-mu fz, -fy-mu fz per
 *                             (step, leg))], CasADi's sign convention.  Mapped on the device to
 *                             this solver's force dual y = F' lam_fric + lam_x[u].
 *   lam_out   [B][52N]  fp32  nullable; the multipliers of the returned point in the same layout:
 *                             H w + g + A' lam_a + lam_x = 0 with lam > 0 on active upper and
 *                             lam < 0 on active lower bounds (lam_a dynamics rows = minus the
 *                             adjoint of the rollout; friction / fz-bound multipliers from the
 *                             accepted face set; swing forces lam_x = -(2R u - Bd' lam_eq)).
 * lam_init may alias lam_out and w_init may alias w_out. */
int cmpc_solve_ref(cmpc_plan* plan, int64_t B, const float* Ad, const float* Bd, const float* gd,
                   const float* x0, const float* xref, const uint8_t* contact,
                   const float* w_init, const float* lam_init, float* w_out, float* lam_out,
                   int32_t* status, int32_t* iters, void* stream);

/* Every argument of a solve in one struct; the entry that takes per-instance terrain.  It covers
 * cmpc_solve, cmpc_solve_warm and cmpc_solve_ref (which are wrappers over the same launch) and
 * adds:
 *   mu      [B]  fp32  nullable; the friction coefficient of instance b (NULL: params.mu)
 *   fz_min  [B]  fp32  nullable; its stance normal-force lower bound (NULL: params.fz_min)
 * The kernels read both arrays when they run, one wave-uniform value per instance: a captured
 * graph sees values the caller has since written in place, and a terrain estimator can change a
 * robot's mu from one tick to the next without a new plan.  NULL, or an array filled with the
 * plan's constant, computes bit for bit what the plan's constant computes.
 * An entry is invalid when mu is not finite, mu <= 0 or fz_min is not finite.  An invalid entry
 * never fails the call: that instance returns status -10 with zero forces and X = the rollout
 * of zero forces (the path an instance with no stance leg takes), its y_out row is zero, and
 * every other instance of the batch is solved as if the entry were valid.
 * Per-instance cost weights, the same way:
 *   Q       [B][12]  fp32  nullable; the state-weight diagonal of instance b (NULL: params.Q)
 *   R       [B][12]  fp32  nullable; its input-weight diagonal (NULL: params.R)
 * in the order of params.Q / params.R.  The kernels read the rows when they run (a captured
 * graph sees values written in place since), and NULL, or rows filled with the plan's
 * constants, compute bit for bit what the plan's constants compute; either array alone may be
 * given.  A row is invalid by the tests cmpc_plan_create applies to the constants: any Q entry
 * negative or not finite, any R entry <= 0 or not finite.  An invalid row is treated as an
 * invalid terrain entry is: status -10, zero forces, X = the rollout of zero forces, a zero
 * y_out / lam_out row, and the rest of the batch solved normally.  The status-1 certificate
 * uses the instance's own strong-convexity modulus min_i 2 R[b][i].
 * `size` is the caller's sizeof of the struct: fields past it are read as NULL, so the struct
 * can grow at its end without an ABI bump.  The inputs Ad..contact and the outputs w_out,
 * status, iters are required; w_init, y_init / y_out and lam_init / lam_out are as for
 * cmpc_solve_warm / cmpc_solve_ref.  The y pair (this solver's dual) and the lam pair (the
 * reference's multipliers) are exclusive: one of each together is CMPC_E_INVALID.
 * Same guarantees as cmpc_solve: asynchronous on `stream`, no allocation, no host
 * synchronisation, graph-capturable. */
typedef struct cmpc_solve_io {
  uint32_t size;            /* sizeof of this struct in the caller's header */
  /* inputs, layouts as cmpc_solve */
  const float *Ad, *Bd, *gd, *x0, *xref;
  const uint8_t* contact;
  const float* mu;          /* [B] nullable */
  const float* fz_min;      /* [B] nullable */
  const float *w_init, *y_init, *lam_init; /* nullable */
  /* outputs */
  float *w_out, *y_out, *lam_out;          /* y_out, lam_out nullable */
  int32_t *status, *iters;
  /* appended after the first release of this struct (a smaller `size` reads them as NULL) */
  const float* Q;           /* [B][12] nullable */
  const float* R;           /* [B][12] nullable */
} cmpc_solve_io;

int cmpc_solve_io_run(cmpc_plan* plan, int64_t B, const cmpc_solve_io* io, void* stream);

/* Cost and KKT residuals of B points of the QP, on the device: how good is each answer of a
 * batch.  Evaluates, for every instance, the reference QP that Ad..contact and the instance's
 * Q, R, mu, fz_min define (H = diag(2Q.., 2R..), g = [-2Q xref; 0], A = [dynamics rows; friction
 * rows], the bounds of centroidal_mpc.py:122-176, 255-283) at the point w with the multipliers
 * lam, in CasADi's convention  H w + g + A' lam_a + lam_x = 0,  lam > 0 only on an active upper
 * and lam < 0 only on an active lower bound:
 *   res[b][CMPC_KKT_COST]  1/2 w'Hw + g'w  (the reference's sol["cost"])
 *   res[b][CMPC_KKT_STAT]  max |H w + g + A' lam_a + lam_x|
 *   res[b][CMPC_KKT_PRIM]  the largest violation of lba <= A w <= uba and lbx <= w <= ubx
 *   res[b][CMPC_KKT_COMP]  the largest  max(lam, 0) |ub - v|  or  max(-lam, 0) |v - lb|  over the
 *                          bounds on v = w (lam_x) and v = A w (lam_a); +inf when a multiplier
 *                          has the sign of an infinite bound (a positive friction multiplier on a
 *                          swing leg, a nonzero lam_x on a state)
 * All arithmetic is fp64 on the fp32 inputs widened exactly; each sum runs in a fixed order, so
 * the results are bitwise repeatable and do not depend on B or on the instance's place in the
 * batch.  Nonzero contact entries are stance.
 *   w    [B][24N]  fp32  the point, in w_out's layout (not modified)
 *   lam  [B][52N]  fp32  nullable; [lam_x | lam_a] in the layout of cmpc_solve_ref's lam_out.
 *                        NULL: the multipliers are first recovered from w on the device (fp64):
 *                        the dynamics rows' from the backward adjoint of the rollout, the
 *                        friction and fz_min multipliers from the faces w's forces hold (a force
 *                        is on a face within face_tol x max(1, |fz|)), a swing force's
 *                        lam_x = -(2R u - Bd' lam_eq).  STAT is then the stationarity left on
 *                        the free force directions, which the solver's status-1 certificate
 *                        does not bound.  This is the mode for the w_out of a solve.
 *   mu, fz_min, Q, R     nullable per-instance values, as in the struct cmpc_solve_io: NULL,
 *                        or rows filled with the plan's constants, give bit for bit the same.
 *                        An instance whose entry is invalid by that struct's rules gets four
 *                        NaNs; it never fails the call and the other instances are unaffected.
 *   face_tol             used when lam == NULL; 0 selects 1e-6.  Negative or not finite:
 *                        CMPC_E_INVALID.
 *   res  [B][4]    fp64  out
 * `size` is the caller's sizeof of the struct (fields past it read as NULL or 0); it must reach
 * past `res`.  B >= 1; no workspace is used, so the plan's max_batch does not limit B.  Same
 * guarantees as cmpc_solve: asynchronous on `stream`, no allocation, no host synchronisation,
 * graph-capturable; the plan's device must be current. */
typedef struct cmpc_kkt_io {
  uint32_t size;            /* sizeof of this struct in the caller's header */
  const float *Ad, *Bd, *gd, *x0, *xref;  /* as cmpc_solve */
  const uint8_t* contact;
  const float *mu, *fz_min; /* [B] nullable: the plan's constants */
  const float *Q, *R;       /* [B][12] nullable */
  const float* w;           /* [B][24N] the point to evaluate (a w_out) */
  const float* lam;         /* [B][52N] nullable: [lam_x | lam_a] */
  float face_tol;           /* used when lam == NULL; 0 selects 1e-6 */
  double* res;              /* [B][4] out: cost, stat, prim, comp */
} cmpc_kkt_io;

#define CMPC_KKT_COST 0
#define CMPC_KKT_STAT 1
#define CMPC_KKT_PRIM 2
#define CMPC_KKT_COMP 3
int cmpc_kkt_run(cmpc_plan* plan, int64_t B, const cmpc_kkt_io* io, void* stream);

/* Feedback gain and value function of B solved instances, on the device: how the forces move
 * when the state moves.  At its optimum the QP is an equality-constrained LQ problem on the
 * faces of the friction pyramid its forces hold, so the MPC law is locally affine,
 * u_0 = K x_0 + kappa.  For every instance the entry fixes a set of held faces, solves
 *   min sum_k (x_{k+1}-xref_k)' Q (x_{k+1}-xref_k) + u_k' R u_k,  x_{k+1} = Ad x_k + Bd_k u_k + gd
 * over the forces that stay on those faces, exactly, by the backward Riccati recursion in fp64
 * on the fp32 inputs widened exactly, and returns
 *   K       [B][12][12]  fp64  K[b][i][j] = d u_0[i] / d x_0[j]   (required)
 *   Vx      [B][12]      fp64  nullable; the gradient in x_0 of the optimal cost 1/2 w'Hw + g'w
 *   Vxx     [B][12][12]  fp64  nullable; its Hessian (symmetric)
 *   u_star  [B][12N]     fp64  nullable; the optimum on the held faces, u_0 .. u_{N-1}
 *   faces_out [B][N][4]  uint8 nullable; the face masks used, [step][leg]
 * Face mask of a stance (step, leg):  bit 0  fz = fz_min;  bit 1  fx = +mu fz;  bit 2  fx = -mu fz;
 * bit 3  fy = +mu fz;  bit 4  fy = -mu fz  (bits 5..7 are ignored).  A swing leg has f = 0
 * whatever its mask, and faces_out holds 0 for it.  Both signs of one axis held mean fz = 0 and
 * that axis zero; a mask is inconsistent only when both signs of an axis are set together with
 * bit 0 and fz_min != 0.
 *   faces   [B][N][4]  uint8  nullable; the held faces given by the caller (w is then ignored)
 *   w       [B][24N]   fp32   nullable; with faces == NULL the masks are read off w's forces by
 *                             the rule of cmpc_kkt_run's recovery: a force is on a face within
 *                             face_tol x max(1, |fz|), the + face of an axis tested before the -
 *                             face.  w and faces both NULL: CMPC_E_INVALID.
 *   face_tol                  used when faces == NULL; 0 selects 1e-6.  Negative or not finite:
 *                             CMPC_E_INVALID.
 *   mu, fz_min, Q, R          nullable per-instance values, as in cmpc_kkt_io.
 * An instance with an inconsistent mask, or with a mu / fz_min entry or Q / R row that is
 * invalid by the rules of cmpc_solve_io, gets NaN in every fp64 output and 0xFF in faces_out; it
 * never fails the call and the other instances are unaffected.  A step without a free force
 * parameter contributes a zero gain.
 * `size` is the caller's sizeof of the struct (fields past it read as NULL or 0); it must reach
 * past `K`.  B >= 1; no workspace is used, so the plan's max_batch does not limit B.  Each sum
 * runs in a fixed order: the results are bitwise repeatable and do not depend on B or on the
 * instance's place in the batch.  Same guarantees as cmpc_solve: asynchronous on `stream`, no
 * allocation, no host synchronisation, graph-capturable; the plan's device must be current. */
typedef struct cmpc_gain_io {
  uint32_t size;            /* sizeof of this struct in the caller's header */
  const float *Ad, *Bd, *gd, *x0, *xref;  /* as cmpc_solve */
  const uint8_t* contact;
  const float *mu, *fz_min; /* [B] nullable: the plan's constants */
  const float *Q, *R;       /* [B][12] nullable */
  const float* w;           /* [B][24N] nullable: the point whose held faces define the law */
  const uint8_t* faces;     /* [B][N][4] nullable: held faces given by the caller */
  float face_tol;           /* used when faces == NULL; 0 selects 1e-6 */
  double* K;                /* [B][12][12] out, required */
  double* Vx;               /* [B][12] nullable */
  double* Vxx;              /* [B][12][12] nullable */
  double* u_star;           /* [B][12N] nullable */
  uint8_t* faces_out;       /* [B][N][4] nullable */
} cmpc_gain_io;

#define CMPC_FACE_FZ_MIN 1
#define CMPC_FACE_FX_POS 2
#define CMPC_FACE_FX_NEG 4
#define CMPC_FACE_FY_POS 8
#define CMPC_FACE_FY_NEG 16
int cmpc_gain_run(cmpc_plan* plan, int64_t B, const cmpc_gain_io* io, void* stream);

/* Gradients of a loss through B solved instances (the backward pass of a differentiable MPC
 * layer), on the device.  The function differentiated is the one cmpc_gain_run solves: for every
 * instance w*(theta) = (x_1..x_N, u_0..u_{N-1}) is the minimiser of 1/2 w'Hw + g'w over the
 * dynamics and the held faces, the face set fixed -- cmpc_gain_io's u_star and its rollout.
 * Given gw = dL/dw for any loss L on that solution, the entry returns dL/dtheta for every input
 * a policy or an estimator can set.  Write the restricted QP as [[H, E'], [E, 0]] [w; nu] =
 * [-g; b], E holding the dynamics rows x_{k+1} - Ad x_k - Bd_k u_k = gd (multipliers nu_k), the
 * held face rows (fz = fz_min;  fx - mu fz = 0 on a +mu face, fx + mu fz = 0 on a -mu face; the
 * same for fy) and f = 0 on swing legs, and solve [[H, E'], [E, 0]] [dw; dnu] = [-gw; 0].  With
 * x_0 = x0 and dx_0 = 0:
 *   g_x0     [B][12]          -Ad' dnu_0
 *   g_xref   [B][N][12]       -2Q o dx_{k+1}
 *   g_gd     [B][12]          -sum_k dnu_k
 *   g_Q      [B][12]          2 sum_k dx_{k+1} o (x_{k+1} - xref_k)
 *   g_R      [B][12]          2 sum_k du_k o u_k
 *   g_mu     [B]              sum over held friction rows r of a leg of sigma_r (nu_r dfz +
 *                             dnu_r fz), sigma = -1 on a +mu face and +1 on a -mu face, fz / dfz
 *                             that leg's entries of w* / dw
 *   g_fz_min [B]              -sum dnu_r over held fz = fz_min rows
 *   g_Ad     [B][12][12]      -sum_k (nu_k dx_k' + dnu_k x_k')
 *   g_Bd     [B][N][12][12]   -(nu_k du_k' + dnu_k u_k')
 * All fp64, all nullable, at least one required (else CMPC_E_INVALID); work that only outputs
 * not asked for need is skipped, and an output is bit for bit the same whichever others are
 * asked for.  g_Q and g_R are the gradients in the weight diagonals of the instance, whether
 * they came from the plan or from a Q / R row; g_mu and g_fz_min likewise.  A leg that holds
 * both signs of an axis is pinned at fz = 0 whatever mu and fz_min are (cmpc_gain_io's mask
 * rule) and contributes nothing to g_mu and g_fz_min.
 *   Ad..contact, mu, fz_min, Q, R, w, faces, face_tol   as in cmpc_gain_io; w and faces both
 *                             NULL: CMPC_E_INVALID
 *   gw       [B][24N]  fp32   required; dL/dw in w_out's layout, states then forces, widened
 *                             exactly
 * The gradient is that of the fp64 optimum on the faces named, not of the fp32 w_out, and it
 * does not see a change of the face set.  An instance with an inconsistent mask, or with a mu /
 * fz_min entry or Q / R row that is invalid by the rules of cmpc_solve_io, gets NaN in every
 * output; it never fails the call and the other instances are unaffected.
 * `size` is the caller's sizeof of the struct (fields past it read as NULL or 0); it must reach
 * past `g_x0`.  B >= 1; no workspace is used, so the plan's max_batch does not limit B.  Each
 * sum runs in a fixed order: the results are bitwise repeatable and do not depend on B or on the
 * instance's place in the batch.  Same guarantees as cmpc_solve: asynchronous on `stream`, no
 * allocation, no host synchronisation, graph-capturable; the plan's device must be current. */
typedef struct cmpc_vjp_io {
  uint32_t size;            /* sizeof of this struct in the caller's header */
  const float *Ad, *Bd, *gd, *x0, *xref;  /* as cmpc_solve */
  const uint8_t* contact;
  const float *mu, *fz_min; /* [B] nullable: the plan's constants */
  const float *Q, *R;       /* [B][12] nullable */
  const float* w;           /* [B][24N] nullable: the point whose held faces define w* */
  const uint8_t* faces;     /* [B][N][4] nullable: held faces given by the caller */
  float face_tol;           /* used when faces == NULL; 0 selects 1e-6 */
  const float* gw;          /* [B][24N] dL/dw, required */
  double* g_x0;             /* [B][12] nullable, as every output */
  double* g_xref;           /* [B][N][12] */
  double* g_gd;             /* [B][12] */
  double* g_Q;              /* [B][12] */
  double* g_R;              /* [B][12] */
  double* g_mu;             /* [B] */
  double* g_fz_min;         /* [B] */
  double* g_Ad;             /* [B][12][12] */
  double* g_Bd;             /* [B][N][12][12] */
} cmpc_vjp_io;
int cmpc_vjp_run(cmpc_plan* plan, int64_t B, const cmpc_vjp_io* io, void* stream);

/* Forward-mode derivatives of B solved instances, on the device: how the whole answer moves when
 * the inputs change.  The function differentiated is cmpc_vjp_io's: w*(theta) = (x_1..x_N,
 * u_0..u_{N-1}), the minimiser of 1/2 w'Hw + g'w over the dynamics and the held faces, the face
 * set fixed.  With the restricted QP written [[H, E'], [E, 0]] [w; nu] = [-g; b] as there (the
 * same rows, the same sign of nu), a change d_theta of the inputs moves the solution by
 *   [[H, E'], [E, 0]] [dw; dnu] = [-(dH w + dg + dE' nu);  db - dE w]
 * which is the same LQ problem with other linear terms:
 *   d_x0     [B][12]          dx_0 = d_x0
 *   d_gd     [B][12]          the offset e_k = d_gd + d_Ad x_k + d_Bd_k u_k of every dynamics row
 *   d_Ad     [B][12][12]      e_k, and -d_Ad' nu_{k+1} on dx_{k+1} (nu_N = 0)
 *   d_Bd     [B][N][12][12]   e_k, and -d_Bd_k' nu_k on du_k
 *   d_xref   [B][N][12]       -2Q o d_xref_k on dx_{k+1}
 *   d_Q      [B][12]          2 d_Q o (x_{k+1} - xref_k) on dx_{k+1}
 *   d_R      [B][12]          2 d_R o u_k on du_k
 *   d_mu     [B]              a held friction row fx - s mu fz = 0 (s = +-1) moves to
 *                             dfx - s mu dfz = s d_mu fz, and its multiplier puts
 *                             -s d_mu nu_r on the leg's dfz; the same for fy
 *   d_fz_min [B]              a held fz = fz_min row moves to dfz = d_fz_min
 * All fp32 of the inputs' shapes, widened exactly, all nullable, at least one required (else
 * CMPC_E_INVALID).  A NULL tangent and an array of zeros give equal results (the sign of a zero
 * may differ); work that only absent tangents need (the costate pass for d_Ad, d_Bd, d_mu; the
 * primal solution where only d_x0, d_xref, d_gd, d_fz_min are given) is skipped.  d_Q, d_R, d_mu
 * and d_fz_min apply to the instance's values whether they came from the plan or from a row.  A
 * swing leg keeps df = 0, and a leg that holds both signs of an axis stays pinned at 0 whatever
 * d_mu and d_fz_min are (cmpc_gain_io's mask rule): their entries of dw are exactly 0.
 *   Ad..contact, mu, fz_min, Q, R, w, faces, face_tol   as in cmpc_gain_io; w and faces both
 *                             NULL: CMPC_E_INVALID
 *   dw       [B][24N]  fp64   required; dx_1..dx_N, then du_0..du_{N-1}
 * The tangent is that of the fp64 optimum on the faces named, not of the fp32 w_out, and it does
 * not see a change of the face set.  An instance with an inconsistent mask, or with a mu / fz_min
 * entry or Q / R row that is invalid by the rules of cmpc_solve_io, gets NaN in its whole row of
 * dw; it never fails the call and the other instances are unaffected.
 * `size` is the caller's sizeof of the struct (fields past it read as NULL or 0); it must reach
 * past `dw`.  B >= 1; no workspace is used, so the plan's max_batch does not limit B.  Each sum
 * runs in a fixed order: the results are bitwise repeatable and do not depend on B or on the
 * instance's place in the batch.  Same guarantees as cmpc_solve: asynchronous on `stream`, no
 * allocation, no host synchronisation, graph-capturable; the plan's device must be current. */
typedef struct cmpc_jvp_io {
  uint32_t size;            /* sizeof of this struct in the caller's header */
  const float *Ad, *Bd, *gd, *x0, *xref;  /* as cmpc_solve */
  const uint8_t* contact;
  const float *mu, *fz_min; /* [B] nullable: the plan's constants */
  const float *Q, *R;       /* [B][12] nullable */
  const float* w;           /* [B][24N] nullable: the point whose held faces define w* */
  const uint8_t* faces;     /* [B][N][4] nullable: held faces given by the caller */
  float face_tol;           /* used when faces == NULL; 0 selects 1e-6 */
  const float* d_x0;        /* [B][12] nullable, as every tangent */
  const float* d_xref;      /* [B][N][12] */
  const float* d_gd;        /* [B][12] */
  const float* d_Q;         /* [B][12] */
  const float* d_R;         /* [B][12] */
  const float* d_mu;        /* [B] */
  const float* d_fz_min;    /* [B] */
  const float* d_Ad;        /* [B][12][12] */
  const float* d_Bd;        /* [B][N][12][12] */
  double* dw;               /* [B][24N] out, required */
} cmpc_jvp_io;
int cmpc_jvp_run(cmpc_plan* plan, int64_t B, const cmpc_jvp_io* io, void* stream);

/* Certified float64 refinement of B solved instances, on the device: a primal-dual active-set
 * loop around cmpc_gain_io's u_star that replaces an answer only when the float64 KKT conditions
 * hold on the whole QP, and reports how far the answer given was from that optimum.
 * Per instance the masks of the held faces are read from `faces` or off w's forces, as
 * cmpc_gain_run does.  Then, for round r = 0, 1, ..:
 *   1. (u, x) = the optimum on the held faces and its float64 rollout (cmpc_gain_io's u_star)
 *   2. the costate pass  p_k = 2Q (x_{k+1} - xref_k) + Ad' p_{k+1},  p_N = 0,  and
 *      g_k = 2R u_k + Bd_k' p_k
 *   3. per stance leg, with (gx, gy, gz) its part of g_k: a held sx mu face of x (sx = +-1) has
 *      the multiplier lam_x = -sx gx, the same for y, a face not held 0, and a held fz face
 *      lam_z = gz - mu (lam_x + lam_y)
 *   4. with us = max(1, max|u|) and gs = us x min_i 2R_i, a face not held is violated when its
 *      row  fx - mu fz, -fx - mu fz, fy - mu fz, -fy - mu fz  or  fz_min - fz  is above
 *      prim_tol x us (where both signs of an axis are, only the larger row counts, the + face on
 *      a tie), and a held face is negative when its multiplier is below -dual_tol x gs
 *   5. neither violated nor negative: certified, stop.  r == max_rounds: stop.  Any face
 *      violated: every violated face is added (adding one sign of an axis clears the other) and
 *      nothing is dropped; otherwise every negative face is dropped.  The new masks equal those
 *      of an earlier round of this instance: stop.
 * Outputs, all of the last round's point:
 *   info      [B]        int32  required.  r >= 0: certified after r repairs.
 *                               CMPC_REFINE_INVALID: a mu / fz_min entry or Q / R row invalid by
 *                               the rules of cmpc_solve_io, or a given mask that holds both signs
 *                               of an axis (every inconsistent mask does).  The refinement never
 *                               creates such a mask and does not certify an apex.
 *                               CMPC_REFINE_ROUNDS: not certified within max_rounds repairs.
 *                               CMPC_REFINE_CYCLE: a set of masks came back.
 *                               A certified point satisfies every constraint within
 *                               prim_tol x us and is the exact optimum on its faces, whose
 *                               multipliers are above -dual_tol x gs.  The QP is strongly convex
 *                               with modulus min_i 2R_i, so its forces are within
 *                               |sum_f min(lam_f, 0) a_f|_2 / min_i 2R_i  (a_f the row of face f)
 *                               of the QP's optimum: a few tens of dual_tol x us.
 *   res       [B][3]     fp64   nullable.  [0] the largest row of a face not held, divided by
 *                               us (0 when none is positive); [1] the most negative multiplier of
 *                               a held face, divided by gs (0 when none is negative);
 *                               [2] max|u - u_in| / max(1, max|u_in|), u_in the forces of w: on a
 *                               certified instance, the measured error of the answer given.  NaN
 *                               when w is NULL.
 *   w64       [B][24N]   fp64   nullable; the point in w_out's layout: the states of the float64
 *                               rollout, then the forces
 *   lam_out   [B][52N]   fp64   nullable; the multipliers [lam_x | lam_a], layout and signs as
 *                               cmpc_solve_ref's lam_out (and cmpc_kkt_run's recovery): lam_a =
 *                               [-p_k | the four friction multipliers per (step, leg)],
 *                               lam_x = -lam_z on a stance fz and -g on a swing force.  Negative
 *                               face multipliers are written as they are.
 *   faces_out [B][N][4]  uint8  nullable; the masks, 0 on a swing leg
 *   w_out     [B][24N]   fp32   nullable; may be w.  Written only for a certified instance, as
 *                               the fp32 rounding of w64; every other row is left untouched, bit
 *                               for bit: the entry never makes an answer worse.
 *   status    [B]        int32  nullable, in/out: set to 1 for a certified instance, untouched
 *                               otherwise
 * An invalid instance gets NaN in res, w64 and lam_out and 0xFF in faces_out; it never fails the
 * call and the other instances are unaffected.
 *   Ad..contact, mu, fz_min, Q, R, faces, face_tol   as in cmpc_gain_io.  w as there, and with
 *                               faces given still the answer res[2] measures.  w and faces both
 *                               NULL: CMPC_E_INVALID.
 *   max_rounds                  the repair limit, 0..16; 0 checks only.  Out of range:
 *                               CMPC_E_INVALID.
 *   prim_tol, dual_tol          0 selects 1e-9.  Negative or not finite: CMPC_E_INVALID.
 * `size` is the caller's sizeof of the struct (fields past it read as NULL or 0); it must reach
 * past `info`.  B >= 1; no workspace is used, so the plan's max_batch does not limit B.  Each sum
 * runs in a fixed order: the results are bitwise repeatable and do not depend on B or on the
 * instance's place in the batch.  Same guarantees as cmpc_solve: asynchronous on `stream`, no
 * allocation, no host synchronisation, graph-capturable; the plan's device must be current. */
typedef struct cmpc_refine_io {
  uint32_t size;            /* sizeof of this struct in the caller's header */
  const float *Ad, *Bd, *gd, *x0, *xref;  /* as cmpc_solve */
  const uint8_t* contact;
  const float *mu, *fz_min; /* [B] nullable: the plan's constants */
  const float *Q, *R;       /* [B][12] nullable */
  const float* w;           /* [B][24N] nullable: the answer to refine */
  const uint8_t* faces;     /* [B][N][4] nullable: held faces given by the caller */
  float face_tol;           /* used when faces == NULL; 0 selects 1e-6 */
  int32_t max_rounds;       /* 0..16 */
  float prim_tol, dual_tol; /* 0 selects 1e-9 */
  int32_t* info;            /* [B] out, required */
  double* res;              /* [B][3] nullable */
  double* w64;              /* [B][24N] nullable */
  double* lam_out;          /* [B][52N] nullable */
  uint8_t* faces_out;       /* [B][N][4] nullable */
  float* w_out;             /* [B][24N] nullable, may be w */
  int32_t* status;          /* [B] nullable, in/out */
} cmpc_refine_io;

#define CMPC_REFINE_INVALID (-1)
#define CMPC_REFINE_ROUNDS (-2)
#define CMPC_REFINE_CYCLE (-3)
#define CMPC_REFINE_MAX_ROUNDS 16
int cmpc_refine_run(cmpc_plan* plan, int64_t B, const cmpc_refine_io* io, void* stream);

void cmpc_plan_destroy(cmpc_plan* plan);

/* QP data on the device: the reference's discrete dynamics
 * (com_trajectory.py:221-286, _continuousDynamics + _discreteDynamics) for B robots, in closed
 * form.  Ac is nilpotent (Ac^2 = 0), so the ZOH of com_trajectory.py:278 is exactly
 * Ad = I + Ac dt, Bd_k = (I dt + Ac dt^2/2) Bc_k, and the 50-sample trapezoid of :281-284 is
 * exact for its linear integrand: gd = (I dt + Ac dt^2/2) gc.  Computed in fp64, stored fp32.
 *   mass    [B]            fp32   go2.data.Ig.mass (com_trajectory.py:39)
 *   inertia [B][3][3]      fp32   I_com_world (com_trajectory.py:40); inverted on the device
 *   r_feet  [B][N][4][3]   fp32   lever arms COM -> foot in the world frame, legs FL FR RL RR
 *                                 (r_*_foot_world[:, k], com_trajectory.py:108-207, 242-245)
 *   xref    [B][N][12]     fp32   as for cmpc_solve; yaw_avg = mean_k xref[b][k][5]
 *                                 (np.average(rpy_traj_world[2, :]), com_trajectory.py:226)
 *   Ad, Bd, gd                    outputs, in cmpc_solve's input layouts
 * N is the plan's horizon; dt > 0 (com_trajectory.py:210, time_step).  Asynchronous on
 * `stream`; the outputs can be passed straight to cmpc_solve on the same stream. */
int cmpc_build_dynamics(cmpc_plan* plan, int64_t B, float dt, const float* mass,
                        const float* inertia, const float* r_feet, const float* xref,
                        float* Ad, float* Bd, float* gd, void* stream);

/* Gradients of a loss through cmpc_build_dynamics, on the device: from dL/dAd and dL/dBd (the
 * fp64 arrays cmpc_vjp_run writes) to dL/d(mass, inertia, r_feet, reference yaw).  The function
 * differentiated is the closed form above evaluated in fp64 on the fp32 inputs widened exactly,
 * not its fp32-rounded outputs.  Per robot, with h2 = dt^2/2:
 *   minv = 1/m,  J = inertia^-1 (all 9 entries of inertia independent, no symmetrisation),
 *   yaw = (1/N) sum_k xref[k][5],  Rt = [[c, s, 0], [-s, c, 0], [0, 0, 1]]  (c = cos yaw, s = sin yaw)
 * and per (step k, leg l), with S = [r_kl]x, W = J S and V = Rt W, the 3x3 blocks of
 * Bd_k[:, 3l:3l+3] are  rows 0-2 h2 minv I3,  rows 3-5 h2 V,  rows 6-8 dt minv I3,
 * rows 9-11 dt W;  Ad[3:6, 9:12] = dt Rt.  Every other entry of Ad, and gd, is constant.
 * With GA = g_Ad, and G0..G3 the blocks of rows 0-2, 3-5, 6-8, 9-11 of g_Bd[k][:, 3l:3l+3]:
 *   g_minv = sum_kl (h2 tr G0 + dt tr G2),            g_mass = -g_minv / m^2
 *   M_kl   = dt G3 + h2 Rt' G1                        (the gradient in W_kl)
 *   g_S    = J' M_kl,   g_r_feet[k][l] = (g_S[2][1] - g_S[1][2], g_S[0][2] - g_S[2][0],
 *                                          g_S[1][0] - g_S[0][1])
 *   g_J    = sum_kl M_kl S',                          g_inertia = -J' g_J J'
 *   g_Rt   = dt GA[3:6, 9:12] + h2 sum_kl G1 W_kl'
 *   g_yaw  = -s g_Rt[0][0] + c g_Rt[0][1] - c g_Rt[1][0] - s g_Rt[1][1]
 * The gradient in xref[b][k][5] is g_yaw[b] / N for every k, in every other entry of xref zero.
 *   mass, inertia, r_feet, xref   as for cmpc_build_dynamics, required
 *   dt                            > 0 and finite, else CMPC_E_INVALID
 *   g_Ad   [B][12][12]    fp64    nullable: read as zeros
 *   g_Bd   [B][N][12][12] fp64    nullable: read as zeros (and then not read at all); 16-byte
 *                                 aligned; g_Ad and g_Bd both NULL: CMPC_E_INVALID
 *   g_mass [B], g_inertia [B][3][3], g_r_feet [B][N][4][3], g_yaw [B]   fp64 outputs, each
 *                                 nullable, at least one required (else CMPC_E_INVALID)
 * An output is bit for bit the same whichever other outputs are asked for; the parts of g_Bd
 * that only absent outputs need are not read.  A NULL g_Ad or g_Bd and an array of zeros give
 * equal results (the sign of a zero may differ).  mass and inertia are not validated, as in
 * cmpc_build_dynamics: a singular inertia gives the Inf or NaN its arithmetic gives, in that
 * robot's rows only.
 * `size` is the caller's sizeof of the struct (fields past it read as NULL); it must reach past
 * `g_mass`.  B >= 0 (B == 0 returns CMPC_OK); no workspace is used, so the plan's max_batch does
 * not limit B.  Each sum runs in a fixed order: the results are bitwise repeatable and do not
 * depend on B or on the robot's place in the batch.  Asynchronous on `stream`, no allocation, no
 * host synchronisation, graph-capturable; the plan's device must be current. */
typedef struct cmpc_dynamics_vjp_io {
  uint32_t size;            /* sizeof of this struct in the caller's header */
  const float *mass, *inertia, *r_feet, *xref;  /* as cmpc_build_dynamics, required */
  float dt;                 /* > 0, finite */
  const double* g_Ad;       /* [B][12][12] nullable: read as zeros */
  const double* g_Bd;       /* [B][N][12][12] nullable: read as zeros; one of the two required */
  double* g_mass;           /* [B] nullable, as every output; one required */
  double* g_inertia;        /* [B][3][3] */
  double* g_r_feet;         /* [B][N][4][3] */
  double* g_yaw;            /* [B] gradient in yaw_avg; d/dxref[b][k][5] = g_yaw[b] / N */
} cmpc_dynamics_vjp_io;
int cmpc_dynamics_vjp_run(cmpc_plan* plan, int64_t B, const cmpc_dynamics_vjp_io* io, void* stream);

/* Forward-mode derivative of cmpc_build_dynamics, on the device: how Ad and Bd move with the
 * mass, the inertia, the foot levers and the reference yaw -- cmpc_dynamics_vjp_io's function
 * and notation, its Jacobian applied from the other side.  The tangents are fp32 of the inputs'
 * shapes, widened exactly; of d_xref only column 5 is read:
 *   dminv = -d_mass / m^2,   dJ = -J d_inertia J,   dyaw = (1/N) sum_k d_xref[k][5]
 *   dRt   = dyaw [[-s, c, 0], [-c, -s, 0], [0, 0, 0]]
 *   dS    = [d_r_kl]x,   dW = dJ S + J dS,   dV = dRt W + Rt dW
 * the blocks of d_Bd_k[:, 3l:3l+3] are  h2 dminv I3,  h2 dV,  dt dminv I3,  dt dW, and
 * d_Ad[3:6, 9:12] = dt dRt with every other entry of d_Ad exactly 0.  The tangent of gd is
 * identically 0 and is not an output.
 *   mass, inertia, r_feet, xref, dt   as in cmpc_dynamics_vjp_io
 *   d_mass [B], d_inertia [B][3][3], d_r_feet [B][N][4][3], d_xref [B][N][12]   fp32, each
 *                                 nullable (an input that does not move), at least one required
 *   d_Ad   [B][12][12]    fp32    nullable output, written whole
 *   d_Bd   [B][N][12][12] fp32    nullable output, 16-byte aligned; d_Ad and d_Bd both NULL:
 *                                 CMPC_E_INVALID
 * Computed in fp64 and rounded once, to the fp32 cmpc_jvp_io's d_Ad and d_Bd take.  An output is
 * bit for bit the same whether or not the other is asked for; a NULL tangent and an array of
 * zeros give equal results (the sign of a zero may differ).  Values are treated as in
 * cmpc_dynamics_vjp_io.  `size` must reach past `d_Ad`; B, the fixed order of every sum, the
 * stream, allocation and capture guarantees are cmpc_dynamics_vjp_run's. */
typedef struct cmpc_dynamics_jvp_io {
  uint32_t size;            /* sizeof of this struct in the caller's header */
  const float *mass, *inertia, *r_feet, *xref;  /* as cmpc_build_dynamics, required */
  float dt;                 /* > 0, finite */
  const float *d_mass, *d_inertia, *d_r_feet, *d_xref;  /* the inputs' shapes, nullable, one
                                                           required; d_xref [B][N][12] */
  float* d_Ad;              /* [B][12][12] nullable; one of the two required */
  float* d_Bd;              /* [B][N][12][12] */
} cmpc_dynamics_jvp_io;
int cmpc_dynamics_jvp_run(cmpc_plan* plan, int64_t B, const cmpc_dynamics_jvp_io* io, void* stream);

/* Reference trajectory, contact table and foot levers on the device: the
 * reference's ComTraj.generate_traj (com_trajectory.py:27-207) up to the dynamics, for B robots,
 * with the Pinocchio quantities it reads passed in (see oracle/traj_ref.py):
 *   x0         [B][12]    fp32   go2.compute_com_x_vec() (com_trajectory.py:37): p, rpy, v, w.
 *                                R_z(x0[5]) is go2.R_z; (R_z R_y R_x)(x0[3:6])' is
 *                                go2.R_world_to_body (go2_robot_data.py:211-222)
 *   pos_des    [B][3]     fp64   in/out: ComTraj.pos_des_world, the per-robot desired position
 *                                (initialise to x0[0:3], com_trajectory.py:12-13); clamped to
 *                                0.1 m of x0 in x/y and set to the commanded z (:47-60)
 *   cmd        [B][4]     fp32   x_vel_des_body, y_vel_des_body, z_pos_des_body,
 *                                yaw_rate_des_body (generate_traj's arguments, :27-35)
 *   t_now      [B]        fp64   time_now (:30)
 *   gait       [B][6]     fp64   gait_period (= 1/frequency_hz), duty, phase offsets FL FR RL RR
 *                                (gait.py:8, 13-19)
 *   foot_lever [B][4][3]  fp32   go2.get_foot_lever_world() (:113, go2_robot_data.py:261-269)
 *   hip        [4][3]     fp32   go2.get_hip_offset(leg), body frame (gait.py:46), all robots
 *   xref       [B][N][12] fp32   out: compute_x_ref_vec() transposed (cmpc_solve's layout)
 *   contact    [B][4][N]  uint8  out: contact_table (:106, gait.py:26-37), bit-identical
 *   r_feet     [B][N][4][3] fp32 out: r_{fl,fr,rl,rr}_foot_world (:108-207), the levers
 *                                cmpc_build_dynamics takes
 * N is the plan's horizon (the reference's int(gait_period / time_step)); dt = time_step > 0.
 * Asynchronous on `stream`; the outputs chain into cmpc_build_dynamics and cmpc_solve. */
int cmpc_generate_traj(cmpc_plan* plan, int64_t B, double dt, const float* x0, double* pos_des,
                       const float* cmd, const double* t_now, const double* gait,
                       const float* foot_lever, const float* hip, float* xref, uint8_t* contact,
                       float* r_feet, void* stream);

/* Gradients of a loss through cmpc_generate_traj, on the device: from dL/dxref (the fp64 g_xref
 * cmpc_vjp_run writes), dL/dr_feet and dL/dyaw_avg (the fp64 g_r_feet and g_yaw
 * cmpc_dynamics_vjp_run writes) and dL/dpos_des' to dL/d(x0, pos_des, cmd, foot_lever).  The
 * function differentiated is what cmpc_generate_traj evaluates before it rounds, in fp64 on the
 * fp32 inputs widened exactly.  The contact table and the stance / take-off pattern depend on
 * t_now and gait alone, are piecewise constant and are held fixed, as is the branch of the clamp:
 * there is no derivative in t_now, gait, hip or dt.  Per robot, with
 *   (px, py, phi, theta, psi) = x0[0, 1, 3, 4, 5],   (vxb, vyb, zdes, wz) = cmd,
 *   t_k = (k + 1) dt,   tau = ((1 - duty) period + 0.5 duty period) / 2,   c, s = cos, sin psi:
 * clamp:     per axis a of x, y  sigma_a = 1 when cmpc_generate_traj clamps (pos_des[a] - p_a > 0.1
 *            or p_a - pos_des[a] > 0.1, strict, in that order), else 0;  pd_a = p_a +- 0.1 when
 *            clamped, else pos_des[a];  pd_z = zdes (pos_des[2] has no effect)
 * reference: vwx = c vxb - s vyb,  vwy = s vxb + c vyb,
 *            xref[k] = (pd_x + vwx t_k, pd_y + vwy t_k, pd_z, 0, 0, psi + wz t_k, vwx, vwy, 0, 0,
 *                       0, wz)
 * levers:    each (k, leg) is of class S (swing at the step's start: r = 0), C (stance, no
 *            take-off at a step <= k: r = foot_lever[leg]) or P (stance, last take-off at step
 *            j <= k), decided as cmpc_generate_traj decides it.  In class P, with
 *            psi_j = psi + wz t_j, (hwx, hwy) = R_z(psi_j) (hip[leg][0], hip[leg][1]),
 *            vbx = cos(theta) vxb, vby = sin(theta) sin(phi) vxb + cos(phi) vyb:
 *              r = (hwx + vbx tau - wz tau hwy,  hwy + vby tau + wz tau hwx,  0.02 - zdes)
 *            (r does not depend on px, py or pos_des: the base position cancels).
 * With G = g_xref, plus g_yaw / N on column 5 of every row when g_yaw is given, H = g_r_feet and
 * gp = g_pos_des_out:
 *   g_pd_a = sum_k G[k][a] + gp[a]                     g_zdes = sum_k G[k][2] + gp[2] - sum_P H[2]
 *   g_vwx  = sum_k (t_k G[k][0] + G[k][6])             g_vwy likewise with columns 1 and 7
 *   g_psi  = sum_k G[k][5]                             g_wz = sum_k (t_k G[k][5] + G[k][11])
 * over class P:  g_vbx += tau H[0],  g_vby += tau H[1],  g_hwx = H[0] + wz tau H[1],
 *   g_hwy = H[1] - wz tau H[0],  g_wz += tau (-hwy H[0] + hwx H[1]),
 *   g_psij = -hwy g_hwx + hwx g_hwy,  g_psi += g_psij,  g_wz += t_j g_psij
 * over class C:  g_foot_lever[leg] += H[k][leg]
 * and then
 *   g_vxb = c g_vwx + s g_vwy + cos(theta) g_vbx + sin(theta) sin(phi) g_vby
 *   g_vyb = -s g_vwx + c g_vwy + cos(phi) g_vby
 *   g_psi += -vwy g_vwx + vwx g_vwy
 *   g_theta = -sin(theta) vxb g_vbx + cos(theta) sin(phi) vxb g_vby
 *   g_phi = (sin(theta) cos(phi) vxb - sin(phi) vyb) g_vby
 *   g_x0 = (sigma_x g_pd_x, sigma_y g_pd_y, 0, g_phi, g_theta, g_psi, 0, 0, 0, 0, 0, 0)
 *   g_pos_des = ((1 - sigma_x) g_pd_x, (1 - sigma_y) g_pd_y, 0)
 *   g_cmd = (g_vxb, g_vyb, g_zdes, g_wz)
 *   x0, cmd, t_now, gait, hip   as for cmpc_generate_traj, required
 *   pos_des       [B][3]  fp64  required, not modified: THE VALUE BEFORE cmpc_generate_traj
 *                               OVERWROTE IT.  cmpc_generate_traj stores the clamped value in
 *                               place; with that value a clamped robot reads as unclamped, and
 *                               its gradient goes to pos_des where it belongs to x0.  Keep a copy.
 *   dt                          > 0 and finite, else CMPC_E_INVALID
 *   g_xref        [B][N][12]    fp64, nullable: read as zeros
 *   g_r_feet      [B][N][4][3]  fp64, nullable: read as zeros
 *   g_yaw         [B]           fp64, nullable: cmpc_dynamics_vjp_io's g_yaw, added as g_yaw / N
 *                               to every step's yaw gradient
 *   g_pos_des_out [B][3]        fp64, nullable: the gradient in the pos_des cmpc_generate_traj
 *                               leaves behind (a loss that reaches the next tick); all four NULL:
 *                               CMPC_E_INVALID
 *   g_x0 [B][12] (written whole), g_pos_des [B][3], g_cmd [B][4], g_foot_lever [B][4][3]   fp64
 *                               outputs, each nullable, at least one required (else
 *                               CMPC_E_INVALID).  foot_lever's values are not needed.
 * An output is bit for bit the same whichever other outputs are asked for.  A NULL gradient and
 * an array of zeros give equal results (the sign of a zero may differ).  Values are not
 * validated: a NaN stays in its robot's rows.
 * `size` is the caller's sizeof of the struct (fields past it read as NULL); it must reach past
 * `g_x0`.  B >= 0 (B == 0 returns CMPC_OK); no workspace is used, so the plan's max_batch does
 * not limit B.  Each sum runs in a fixed order: the results are bitwise repeatable and do not
 * depend on B or on the robot's place in the batch.  Asynchronous on `stream`, no allocation, no
 * host synchronisation, graph-capturable; the plan's device must be current. */
typedef struct cmpc_traj_vjp_io {
  uint32_t size;            /* sizeof of this struct in the caller's header */
  const float* x0;          /* [B][12] required, as the other inputs */
  const double* pos_des;    /* [B][3] the value BEFORE cmpc_generate_traj's clamp; not modified */
  const float* cmd;         /* [B][4] */
  const double* t_now;      /* [B] */
  const double* gait;       /* [B][6] */
  const float* hip;         /* [4][3] */
  double dt;                /* > 0, finite */
  const double* g_xref;     /* [B][N][12] nullable: read as zeros, as the next three; one required */
  const double* g_r_feet;   /* [B][N][4][3] */
  const double* g_yaw;      /* [B] gradient in the mean reference yaw, spread as g_yaw / N */
  const double* g_pos_des_out; /* [B][3] gradient in the pos_des cmpc_generate_traj leaves */
  double* g_x0;             /* [B][12] nullable, as every output; one required */
  double* g_pos_des;        /* [B][3] */
  double* g_cmd;            /* [B][4] */
  double* g_foot_lever;     /* [B][4][3] */
} cmpc_traj_vjp_io;
int cmpc_traj_vjp_run(cmpc_plan* plan, int64_t B, const cmpc_traj_vjp_io* io, void* stream);

/* Forward-mode derivative of cmpc_generate_traj, on the device: how xref, r_feet and the pos_des
 * it leaves move with x0, pos_des, cmd and foot_lever -- cmpc_traj_vjp_io's function and
 * notation, its Jacobian applied from the other side.  With d_vxb, d_vyb, d_zdes, d_wz = d_cmd
 * and dp, dphi, dtheta, dpsi from d_x0 (only its entries 0, 1, 3, 4, 5 are read):
 *   dvwx = c d_vxb - s d_vyb - vwy dpsi,   dvwy = s d_vxb + c d_vyb + vwx dpsi
 *   dpd_a = sigma_a dp_a + (1 - sigma_a) d_pos_des[a],   dpd_z = d_zdes
 *   d_xref[k] = (dpd_x + dvwx t_k, dpd_y + dvwy t_k, d_zdes, 0, 0, dpsi + d_wz t_k, dvwx, dvwy,
 *                0, 0, 0, d_wz)
 *   dvbx = cos(theta) d_vxb - sin(theta) vxb dtheta
 *   dvby = (cos(theta) sin(phi) dtheta + sin(theta) cos(phi) dphi) vxb + sin(theta) sin(phi) d_vxb
 *          - sin(phi) vyb dphi + cos(phi) d_vyb
 *   class P, with dpsi_j = dpsi + d_wz t_j, dhwx = -hwy dpsi_j, dhwy = hwx dpsi_j:
 *     d_r = (dhwx + tau dvbx - tau (d_wz hwy + wz dhwy),
 *            dhwy + tau dvby + tau (d_wz hwx + wz dhwx),  -d_zdes)
 *   class C: d_r = d_foot_lever[leg];   class S: exactly 0
 *   d_pos_des_out = (dpd_x, dpd_y, d_zdes)
 *   x0, pos_des (before the clamp), cmd, t_now, gait, hip, dt   as in cmpc_traj_vjp_io
 *   d_x0 [B][12] fp32, d_pos_des [B][3] fp64, d_cmd [B][4] fp32, d_foot_lever [B][4][3] fp32
 *                               each nullable (an input that does not move), at least one required
 *   d_xref        [B][N][12]    fp32 nullable output; columns 3, 4, 8, 9, 10 are exactly 0
 *   d_r_feet      [B][N][4][3]  fp32 nullable output
 *   d_pos_des_out [B][3]        fp64 nullable output; all three NULL: CMPC_E_INVALID
 * The two fp32 outputs are computed in fp64 and rounded once: they are what cmpc_jvp_io's d_xref
 * and cmpc_dynamics_jvp_io's d_r_feet and d_xref take.  An output is bit for bit the same
 * whichever others are asked for; a NULL tangent and an array of zeros give equal results (the
 * sign of a zero may differ).  Values are treated as in cmpc_traj_vjp_io.  `size` must reach past
 * `d_xref`; B, the stream, allocation and capture guarantees are cmpc_traj_vjp_run's. */
typedef struct cmpc_traj_jvp_io {
  uint32_t size;            /* sizeof of this struct in the caller's header */
  const float* x0;          /* [B][12] required, as the other inputs */
  const double* pos_des;    /* [B][3] the value BEFORE cmpc_generate_traj's clamp; not modified */
  const float* cmd;         /* [B][4] */
  const double* t_now;      /* [B] */
  const double* gait;       /* [B][6] */
  const float* hip;         /* [4][3] */
  double dt;                /* > 0, finite */
  const float* d_x0;        /* [B][12] nullable, as the next three; one required */
  const double* d_pos_des;  /* [B][3] */
  const float* d_cmd;       /* [B][4] */
  const float* d_foot_lever; /* [B][4][3] */
  float* d_xref;            /* [B][N][12] nullable, as every output; one required */
  float* d_r_feet;          /* [B][N][4][3] */
  double* d_pos_des_out;    /* [B][3] */
} cmpc_traj_jvp_io;
int cmpc_traj_jvp_run(cmpc_plan* plan, int64_t B, const cmpc_traj_jvp_io* io, void* stream);

/* The reference's 1 kHz leg controller for B robots (the consumer of the
 * QP's first forces): LegController.compute_leg_torque for legs FL FR RL RR
 * (leg_controller.py:43-112; test_MPC.py:199-225) -- stance tau = J_foot' (-f) (:100-101),
 * swing tau = J_foot' (KP e_p + KD e_v + Lambda (a_des - Jdot dq)) + (C dq + g)[leg] with
 * Lambda = (J_full M^-1 J_full')^-1 (:75-98) and the swing trajectory planned at take-off
 * (gait.py:77-174) -- then clipped to +-tau_max (test_MPC.py:227-228; tau_max <= 0: no clip).
 * Pinocchio's quantities are inputs (fp64, as the reference computes them):
 *   t        [B]           time_now;  gait [B][6] as for cmpc_generate_traj
 *   force    fp32 rows of 12, row stride force_stride (>= 12) floats: U[:, 0] of each robot,
 *            e.g. w_out + 12 N with stride 24 N (test_MPC.py:196)
 *   J_foot   [B][4][3][3]  compute_3x3_foot_Jacobian_world(leg) (go2_robot_data.py:286-301)
 *   J_full   [B][4][3][18] compute_full_foot_Jacobian_world(leg) (:347-353)
 *   M, C     [B][18][18]   compute_dynamcis_terms() (:355-360);  g, dq [B][18]
 *   Jdot_dq, foot_pos, foot_vel [B][4][3]  compute_Jdot_dq_world, get_single_foot_state_in_world
 *   body     [B][16]  base_pos(3), pos_com_world(3), vel_com_world(3), yaw (R_z),
 *                     yaw_rate_des_world, x/y_pos_des_world, x/y_vel_des_world, 0
 *                     (what gait.py:80-96 reads; the des values generate_traj stored)
 *   hip      [4][3]   get_hip_offset(leg)
 *   state    [B][4][8] in/out, the controller's memory: last mask (initialise to 2), take-off
 *                     time, swing start (3), touchdown (3)  (leg_controller.py:41, 67-72, 104)
 *   tau      [B][12]  out, fp64. */
int cmpc_leg_torque(cmpc_plan* plan, int64_t B, const double* t, const double* gait,
                    const float* force, int64_t force_stride, const double* J_foot,
                    const double* J_full, const double* M, const double* C, const double* g,
                    const double* dq, const double* Jdot_dq, const double* foot_pos,
                    const double* foot_vel, const double* body, const double* hip,
                    double* state, double tau_max, double* tau, void* stream);

/* Closed-loop stand-in for the simulator (MuJoCo is absent from this image):
 * advance B single-rigid-body robots by nsub substeps of dt under the held ground forces U[:, 0]
 * (rows of 12 fp32, row stride force_stride), with the gait deciding contact at each substep.
 *   t_now [B] fp64 (start time, not advanced), gait [B][6] as above, mass [B],
 *   inertia_body [B][3][3] (body-frame I_com), hip [4][3];
 *   x [B][12] in/out (p, rpy, v, w_world: the MPC state), feet [B][4][3] in/out (world foot
 *   positions, used while in stance), contact_state [B] in/out (bit l: leg l in stance).
 * Not a reference interface: it exists to exercise the on-device tick in closed loop. */
int cmpc_srb_step(cmpc_plan* plan, int64_t B, int nsub, double dt, const double* t_now,
                  const double* gait, const float* mass, const float* inertia_body,
                  const float* force, int64_t force_stride, const float* hip, float* x,
                  float* feet, uint8_t* contact_state, void* stream);

/* cmpc_srb_step with two options: the first-order MPC force law applied at every substep, and an
 * external wrench.  With neither, and no output asked for, it is cmpc_srb_step bit
 * for bit.  The substep is cmpc_srb_step's with two additions.
 *
 * Force law.  With x_s the fp32 state at a substep's start, a robot that has the law applies
 *   delta = x_s - x_solve                     in fp32, widened to fp64
 *   u_i   = fl32(U0_i + sum_j K_ij delta_j)    in fp64, j = 0 .. 11 in that order, U0 first
 * and, for each leg l with contact[b][l][0] != 0 (the MPC's stance at step 0),
 *   fz = max(u_z, fz_min),  fx = min(max(u_x, -mu fz), mu fz),  fy likewise (the clamped fz).
 * A leg with contact[b][l][0] == 0 keeps its U0 triple: no feedback, no clamp, so a leg the MPC
 * planned in swing never receives fz_min.  Which legs apply their force is still decided by the
 * gait at the substep time, as in cmpc_srb_step.
 * A robot holds U0 for the whole call and gets fb_status 0 when K is NULL, when its K block has
 * an entry that is not finite (cmpc_gain_run writes NaN for an inconsistent face mask), or when
 * its mu or fz_min is invalid by cmpc_solve_io's rules (mu not finite or <= 0, fz_min not
 * finite).  fb_status 1: the law was applied; 2: and at least one clamp changed a component of a
 * force that a leg in stance by the gait applied, in at least one substep.  force_out receives
 * the 12 forces of the last substep before the gait gates them (a held robot's: U0).
 *
 * Wrench.  wrench[b][0:3] is added to the force sum F and wrench[b][3:6] to the torque sum T of
 * every substep, whatever the contacts: a world force at the COM and a world torque about it.
 *
 *   nsub .. contact_state   as for cmpc_srb_step, with its checks
 *   K        [B][12][12] fp64, cmpc_gain_run's K; 16-byte aligned; needs x_solve and contact
 *            (else CMPC_E_INVALID)
 *   x_solve  [B][12]  the state the forces were solved from
 *   contact  [B][4][N] the solve's contact table, N the plan's
 *   mu, fz_min [B], NULL: the plan's constants
 * Neither the solve's status nor friction at the feet enters; there is no derivative entry for
 * the options (cmpc_srb_vjp_run and cmpc_srb_jvp_run differentiate the hold-force plant).
 * `size` is the caller's sizeof of the struct (fields past it read as NULL or 0); it must reach
 * past `contact_state`.  B >= 0 (B == 0 or nsub == 0 returns CMPC_OK with nothing written); no
 * workspace is used, so the plan's max_batch does not limit B; rows past B are untouched.  Every
 * sum runs in one thread in a fixed order: the results are bitwise repeatable and do not depend on
 * B or on the robot's row.  Asynchronous on `stream`, no allocation, no host synchronisation,
 * graph-capturable; the plan's device must be current. */
typedef struct cmpc_srb_io {
  uint32_t size;               /* sizeof of this struct in the caller's header */
  int32_t nsub;                /* as cmpc_srb_step's, as the fields down to contact_state */
  double dt;
  const double* t_now;         /* [B] */
  const double* gait;          /* [B][6] */
  const float* mass;           /* [B] */
  const float* inertia_body;   /* [B][3][3] */
  const float* force;          /* rows of 12, row stride force_stride floats */
  int64_t force_stride;        /* >= 12 */
  const float* hip;            /* [4][3] */
  float* x;                    /* [B][12] in/out */
  float* feet;                 /* [B][4][3] in/out */
  uint8_t* contact_state;      /* [B] in/out */
  /* options, all nullable */
  const double* K;             /* [B][12][12] fp64: cmpc_gain_run's K */
  const float* x_solve;        /* [B][12]: the state the forces were solved from */
  const uint8_t* contact;      /* [B][4][N]: the solve's contact table (N the plan's) */
  const float* mu;             /* [B]; NULL: the plan's constant */
  const float* fz_min;         /* [B]; NULL: the plan's constant */
  const float* wrench;         /* [B][6]: world force at the COM, world torque about it */
  float* force_out;            /* [B][12] out: the law's forces at the last substep */
  uint8_t* fb_status;          /* [B] out: 0 held, 1 law applied, 2 law applied and clamped */
} cmpc_srb_io;
int cmpc_srb_step_io_run(cmpc_plan* plan, int64_t B, const cmpc_srb_io* io, void* stream);

/* Gradients of a loss through cmpc_srb_step, on the device: from dL/dx' and dL/dfeet' to the
 * gradients in the state, the feet, the held forces, the mass and the body inertia.  The function
 * differentiated is the plant's documented model evaluated in fp64 on the fp32
 * inputs widened exactly -- not srb_kernel's fp32 arithmetic.  Per robot, with the state
 * (p, e = rpy, v, w), the feet c_l, ts = duty period (fp64), g = (0, 0, -9.81) and h = dt; t starts
 * at t_now and advances by repeated addition of h.  One substep:
 *   1. sigma_l = stance_at(t, period, duty, offset_l).  A leg with sigma_l set that was not in
 *      stance before (before the first substep: contact_state) lands:
 *        c_l = (p_x + cy hx - sy hy + v_x ts / 2,  p_y + sy hx + cy hy + v_y ts / 2,  0)
 *      with (hx, hy) = hip[l] and the substep's starting p, yaw and v.
 *   2. R = Rz Ry Rx (e), Iw = R Ib R', F = sum sigma f_l, T = sum sigma (c_l - p) x f_l,
 *      y = Iw w, alpha = Iw^-1 (T - w x y): a general 3 x 3 inverse, all 9 entries of Ib
 *      independent, no symmetrisation (as in cmpc_dynamics_vjp_io).
 *   3. v' = v + h (F / m + g),  w' = w + h alpha,  p' = p + h v',  e' = e + h E(e) w', E the ZYX
 *      rate map at the substep's starting e:
 *        roll' = (cy wx + sy wy) / cp,  pitch' = -sy wx + cy wy,  yaw' = wz + sp roll'.
 * The stance pattern and the landings depend on t_now, gait and contact_state alone, so they are
 * piecewise constant: there is no derivative in t_now, gait, hip or dt, and the derivative in
 * everything else is exact, not a held-branch approximation.  The tangent of a substep:
 *   dR = sum_i dR/de_i de_i,   dIw = dR Ib R' + R dIb R' + R Ib dR'
 *   dT = sum sigma [(dc_l - dp) x f_l + (c_l - p) x df_l]
 *   dalpha = Iw^-1 (dT - dw x y - w x (dIw w + Iw dw) - dIw alpha)
 *   dv' = dv + h (sum sigma df_l / m - F dm / m^2),  dw' = dw + h dalpha,  dp' = dp + h dv'
 *   de' = de + h (dE[de] w' + E dw')
 *   at a landing: dc_l = (dp_x - (sy hx + cy hy) dpsi + dv_x ts / 2,
 *                         dp_y + (cy hx - sy hy) dpsi + dv_y ts / 2,  0),
 *   which replaces the leg's previous tangent; a foot that does not land keeps dc_l.
 * The reverse pass is the transpose of that, applied from the last substep to the first; within a
 * substep the landing comes after the dynamics: the leg's foot adjoint flows into p_x, p_y, psi,
 * v_x, v_y of the substep's start and is then zero.
 *   t_now, gait, mass, inertia_body, hip, nsub, dt   as for cmpc_srb_step, required
 *   force, force_stride (>= 12)   as for cmpc_srb_step (w_out + 12 N with stride 24 N works)
 *   x [B][12] fp32, feet [B][4][3] fp32, contact_state [B] uint8   required, not modified: THE
 *                               VALUES BEFORE cmpc_srb_step OVERWROTE THEM.  cmpc_srb_step
 *                               advances all three in place; with the advanced values the
 *                               derivative is that of the next tick.  Keep a copy.
 *   nsub                        1 .. CMPC_SRB_GRAD_MAX_NSUB, else CMPC_E_INVALID
 *   dt                          > 0 and finite, else CMPC_E_INVALID
 *   g_x_out    [B][12]          fp64, nullable: read as zeros
 *   g_feet_out [B][4][3]        fp64, nullable: read as zeros; both NULL: CMPC_E_INVALID
 *   g_x [B][12], g_feet [B][4][3], g_force [B][12] (packed), g_mass [B], g_inertia_body [B][3][3]
 *                               fp64 outputs, each nullable, at least one required (else
 *                               CMPC_E_INVALID)
 * An output is bit for bit the same whichever other outputs are asked for.  A NULL gradient and
 * an array of zeros give equal results (the sign of a zero may differ).  g_force of a leg that is
 * in swing at every substep is exactly 0; g_feet of a leg that is never in stance before it lands
 * is exactly 0, and without a landing it is g_feet_out plus the lever terms.  Values are not
 * validated, as in cmpc_srb_step: a pitch of +-pi/2 or a singular Iw gives the Inf or NaN the
 * arithmetic gives, in that robot's rows only.
 * `size` is the caller's sizeof of the struct (fields past it read as NULL); it must reach past
 * `g_x`.  B >= 0 (B == 0 returns CMPC_OK); no workspace is used, so the plan's max_batch does not
 * limit B.  Every sum runs in a fixed order: the results are bitwise repeatable and do not depend
 * on B or on the robot's place in the batch.  Asynchronous on `stream`, no allocation, no host
 * synchronisation, graph-capturable; the plan's device must be current. */
#define CMPC_SRB_GRAD_MAX_NSUB 64
typedef struct cmpc_srb_vjp_io {
  uint32_t size;               /* sizeof of this struct in the caller's header */
  const double* t_now;         /* [B] required, as the other inputs */
  const double* gait;          /* [B][6] */
  const float* mass;           /* [B] */
  const float* inertia_body;   /* [B][3][3] */
  const float* force;          /* rows of 12, row stride force_stride floats */
  int64_t force_stride;        /* >= 12 */
  const float* hip;            /* [4][3] */
  const float* x;              /* [B][12] the value BEFORE cmpc_srb_step; not modified */
  const float* feet;           /* [B][4][3] likewise */
  const uint8_t* contact_state; /* [B] likewise */
  int32_t nsub;                /* 1 .. CMPC_SRB_GRAD_MAX_NSUB */
  double dt;                   /* > 0, finite */
  const double* g_x_out;       /* [B][12] nullable: read as zeros, as the next; one required */
  const double* g_feet_out;    /* [B][4][3] */
  double* g_x;                 /* [B][12] nullable, as every output; one required */
  double* g_feet;              /* [B][4][3] */
  double* g_force;             /* [B][12] packed */
  double* g_mass;              /* [B] */
  double* g_inertia_body;      /* [B][3][3] */
} cmpc_srb_vjp_io;
int cmpc_srb_vjp_run(cmpc_plan* plan, int64_t B, const cmpc_srb_vjp_io* io, void* stream);

/* Forward-mode derivative of cmpc_srb_step, on the device: how x' and feet' move with x, feet, the
 * held forces, the mass and the body inertia -- cmpc_srb_vjp_io's function and notation, its
 * Jacobian applied from the other side, primal and tangent advanced together in fp64.
 *   t_now .. dt                 as in cmpc_srb_vjp_io: x, feet, contact_state before the step
 *   d_x [B][12], d_feet [B][4][3], d_force [B][12] (packed), d_mass [B], d_inertia_body [B][3][3]
 *                               fp32, widened exactly, each nullable (an input that does not
 *                               move), at least one required
 *   d_x_out    [B][12]          fp32 nullable output
 *   d_feet_out [B][4][3]        fp32 nullable output; both NULL: CMPC_E_INVALID
 * The outputs are computed in fp64 and rounded once: d_x_out is what cmpc_jvp_io's and
 * cmpc_traj_jvp_io's d_x0 take at the next tick, and d_feet_out minus d_x_out's position what
 * cmpc_traj_jvp_io's d_foot_lever takes.  An output is bit for
 * bit the same whichever other is asked for; a NULL tangent and an array of zeros give equal
 * results (the sign of a zero may differ).  d_feet_out of a leg that neither lands nor has a
 * d_feet is exactly 0.  Values are treated as in cmpc_srb_vjp_io.  `size` must reach past
 * `d_x_out`; B, the stream, allocation and capture guarantees are cmpc_srb_vjp_run's. */
typedef struct cmpc_srb_jvp_io {
  uint32_t size;               /* sizeof of this struct in the caller's header */
  const double* t_now;         /* [B] required, as the other inputs */
  const double* gait;          /* [B][6] */
  const float* mass;           /* [B] */
  const float* inertia_body;   /* [B][3][3] */
  const float* force;          /* rows of 12, row stride force_stride floats */
  int64_t force_stride;        /* >= 12 */
  const float* hip;            /* [4][3] */
  const float* x;              /* [B][12] the value BEFORE cmpc_srb_step; not modified */
  const float* feet;           /* [B][4][3] likewise */
  const uint8_t* contact_state; /* [B] likewise */
  int32_t nsub;                /* 1 .. CMPC_SRB_GRAD_MAX_NSUB */
  double dt;                   /* > 0, finite */
  const float* d_x;            /* [B][12] nullable, as the next four; one required */
  const float* d_feet;         /* [B][4][3] */
  const float* d_force;        /* [B][12] packed */
  const float* d_mass;         /* [B] */
  const float* d_inertia_body; /* [B][3][3] */
  float* d_x_out;              /* [B][12] nullable, as the next; one required */
  float* d_feet_out;           /* [B][4][3] */
} cmpc_srb_jvp_io;
int cmpc_srb_jvp_run(cmpc_plan* plan, int64_t B, const cmpc_srb_jvp_io* io, void* stream);

/* Measurement hooks (not on the reference's interface; used by bench.py).  A solve launches at
 * most CMPC_NUM_SOLVE_KERNELS persistent solve kernels; cmpc_plan_solve_kernel names solve
 * kernel k (0, 1 or 2) of a batch of B instances, or returns NULL if that slot is not launched:
 *   B <= cmpc_plan_team_batch:  "solve_team_kernel<4, 1>" (B <= CUs: one workgroup per CU)
 *                               or "solve_team_kernel<4, 2>" (k = 0 only);
 *   larger batches:             "solve_group_kernel<128, 96>" (k = 0, the NC <= 128
 *                               class), "solve_group_kernel<160, 144>" (k = 1, the
 *                               NC 144 / 160 class; NULL if N is too short to need it) and
 *                               "solve_group_kernel<192, 0>" (k = 2, the NC 192 bin, more
 *                               than 160 free forces; NULL if N is too short).  Slots are
 *                               per kernel, whichever class is submitted first
 *                               (cmpc_plan_set_heavy_first).
 * While enabled, cmpc_solve records a hipEvent pair around each solve-kernel launch on the
 * stream it is launched on -- for slot 2 only the NC 192 kernel's early launch (a few waves on
 * the highest-priority plan stream, submitted before the classes); its overflow launch, which
 * drains what those waves left after both classes are done, is not timed.  An event pair spans
 * the launch's queueing too: with an empty bin the early launch's waves exit at once, but they
 * are dispatched only when the class kernels free a SIMD, so that span can read milliseconds
 * while holding nothing.  cmpc_plan_timing_read waits for the recorded events, returns the
 * summed milliseconds per kernel slot (ms_per_kernel[CMPC_NUM_SOLVE_KERNELS]) and the launch
 * counts since the last read, and resets them.  At most 4096 x CMPC_NUM_SOLVE_KERNELS launches
 * are recorded between reads (later ones are not timed). */
#define CMPC_NUM_SOLVE_KERNELS 3
int cmpc_plan_set_timing(cmpc_plan* plan, int enable);
int cmpc_plan_timing_read(cmpc_plan* plan, float* ms_per_kernel, int32_t* calls_per_kernel);
const char* cmpc_plan_solve_kernel(const cmpc_plan* plan, int64_t B, int k);

/* Small-batch mode.  A solve of B <= max_batch instances runs each QP on a workgroup of four
 * waves (one per SIMD of a CU) that split the condensation, the inversion and the matrix-vector
 * products, instead of one wave per QP: B = 256 on 256 CUs otherwise leaves 3 of every 4 SIMDs
 * idle.  All five bins then run in one kernel on `stream` (timed as solve kernel 0).  Results
 * are the same algorithm's (parity-tested in both modes).  max_batch = -1 (the default) selects
 * it for B <= 4 x CUs; 0 disables it.  cmpc_plan_team_batch returns the effective bound. */
int cmpc_plan_set_team(cmpc_plan* plan, int64_t max_batch);
int cmpc_plan_team_batch(const cmpc_plan* plan, int64_t* max_batch);

/* Launch order of the two register classes.  A batch above the small-batch bound launches one
 * persistent kernel per register class (NC <= 128: two waves per SIMD; NC 144 / 160: one; plus
 * the NC 192 bin's kernel, submitted before both on its own stream); the
 * class submitted first fills the device and the other takes SIMDs as they free up, so the
 * step ends with the tail of the class that runs second.  Batches of B >= min_batch submit the
 * NC 144 / 160 class first (its tail is then filled by NC <= 128 waves: config 3 at 65,536 and
 * 16,384 faster), smaller ones the NC <= 128 class (config 2 at 4,096 faster).  Results do not
 * depend on the order (each instance is solved by one wave, deterministically).
 * min_batch = -1 (the default) selects B > 16 x CUs; 0 never.  cmpc_plan_heavy_first_batch
 * returns the effective bound (0: never). */
int cmpc_plan_set_heavy_first(cmpc_plan* plan, int64_t min_batch);
int cmpc_plan_heavy_first_batch(const cmpc_plan* plan, int64_t* min_batch);

/* Acceptance statistics (not on the reference's interface; bench.py reports them): cumulative
 * counts over every solve with this plan since creation or the last reset, read after a device
 * synchronisation:
 *   out[0]  loose acceptances (a polish session that ended on a face set within 5 x polish_tol);
 *   out[1]  answers returned as status 2 because the certified face bound was missed;
 *   out[2]  KKT checks that ran on a refinement that had stopped contracting on a face-downdated
 *           factorization (its step no longer bounds the error): each time the face set was
 *           refactored and the check redone on a fresh refinement;
 *   out[3]  reserved (0).
 * reset != 0 zeroes the counters after reading.  The copy and the reset run on the plan's own
 * stream, never on the null stream (a null-stream operation from the library slowed the
 * caller's later HIP-graph replays). */
#define CMPC_NUM_STATS 4
int cmpc_plan_stats(cmpc_plan* plan, uint64_t* out, int reset);

/* Thread-local description of the last error returned on this thread ("" if none). */
const char* cmpc_last_error(void);

/* Build / ABI identification, e.g. "cmpc 1 gfx950". */
const char* cmpc_version(void);

#ifdef __cplusplus
}
#endif

#endif /* CMPC_H_ */
