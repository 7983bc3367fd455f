"""Float64 reference of the documented ADMM iteration (TEST INFRASTRUCTURE).

Plain NumPy in float64 on the fp32-rounded inputs, independent of tests/algo_spec.py: the QP is
condensed densely (P and q formed from the rollout's linear map), the x-update is solved exactly,
and every definition is the one include/cmpc.h states (cmpc_params: rho, adaptive_rho_interval;
status 2 / -2).

Per instance, on the stance forces u (free-force count n = 3 x stance (step, leg) pairs), with the
cost sum_k (x_{k+1} - xref_k)' Q (x_{k+1} - xref_k) + u_k' R u_k and x_{k+1} = Ad x_k + Bd_k u_k + gd:

    X = G u + c            (the rollout; G from the powers of Ad, c the rollout of zero forces)
    P = 2 (G' Qbar G + Rbar),  q = 2 G' Qbar (c - xref)

From the cold start x = z = y = 0, iteration i = 1, 2, ... at the rho in force:

    g   = P x + q                                      (the gradient at the x before the update)
    x~  = (P + (sigma + rho) I)^-1 (sigma x + rho z - q - y)
    x_r = alpha x~ + (1 - alpha) z
    x   <- alpha x~ + (1 - alpha) x
    z   <- Pi_K(x_r + y / rho),   K = {fz >= fz_min, |fx|, |fy| <= mu fz} per stance leg
    y   <- y + rho (x_r - z)
    rp = |x - z|_inf, rd = |g + y|_inf, np = max(|x|_inf, |z|_inf), nd = max(|g|_inf, |y|_inf)

The start rho is rho0 for n <= 96 and rho0 / 2 above.  At an iteration that is a multiple of
adaptive_rho_interval and not the last (i < max_iter): rho' = clip(rho sqrt((rp / np) / (rd / nd)),
1e-6, 1e6), taken when rho' > 5 rho or rho' < rho / 5.  Exit without a polish: status 2 when
rp <= eps_abs + eps_rel np and rd <= eps_abs + eps_rel nd on the last iteration's values, else -2.
"""
from __future__ import annotations

import numpy as np

Q_DEFAULT = (1, 1, 50, 10, 20, 1, 2, 2, 1, 1, 1, 1)
R_DEFAULT = (1e-5,) * 12
RHO_LOW_ABOVE = 96      # bins with more than this many free forces start at rho0 / 2

# D_k: the worst deviation of the fp32 model's z_k (tests/algo_spec.py, fp32_admm=True) from this
# reference's over test_gpu_admm_passes.batch(16), relative to S = max(1, max|z_ref|), with 10 %
# headroom over the values tests/test_admm_ref.py measures (and asserts).  The bar of the GPU
# tests at iteration k is BAR_FACTOR x D_k.
D_K = {1: 2.0e-4, 2: 8.2e-5, 3: 9.2e-5, 5: 3.5e-5, 8: 8.4e-6, 30: 1.0e-6}
BAR_FACTOR = 4.0
# The same deviation at the two off-default values where the fp32 model itself leaves D_K, over
# the `main` batch of batches() (22 instances, the one the GPU runs), same headroom:
#   alpha = 1.9: the over-relaxed iteration damps an error injected by one fp32 x-update by
#     only |1 - alpha| = 0.9 per iteration (0.6 at the default), so the errors of all k
#     iterations add up instead of decaying (D grows with k);
#   rho = 1e-5: P + (sigma + rho) I is conditioned worse (P's smallest eigenvalues are 2 R =
#     2e-5), so the fp32 factor is a worse inverse in the first iterations, whose steps are large.
D_OFF = {("alpha", 1.9): {1: 3.0e-4, 3: 3.7e-4, 8: 5.0e-4},
         ("rho", 1e-5): {1: 6.5e-4, 3: 4.7e-4, 8: 5.6e-5}}
# y_out's bar gets a floor of this many float32 roundings of a term of size max|q|: y converges to
# -g on the held faces, and g = P x + q is summed in float32 from terms of size |q| (0.3 .. 0.7
# here) while g itself is 100 x smaller; at k = 30 the bar 4 D_k rho S is below one such rounding.
Y_FLOOR_ROUNDINGS = 4
# The float32 evaluation of the lam_out formulas against the float64 one at the reference's z_k,
# relative to the instance's largest multiplier (measured and asserted by tests/test_admm_ref.py,
# same headroom); the GPU bar is BAR_FACTOR x this.
LAM_D = 4.2e-5


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def project(v, mu, fz_min):
    """Euclidean projection of triples (fx, fy, fz) (..., 3) onto K; returns (p, code) with code
    bits 1 fz at fz_min, 2 / 4 fx at +/- mu fz, 8 / 16 fy alike.  K = {|fx|, |fy| <= mu fz}
    intersected with fz >= fz_min; the cone part is piecewise linear in fz (both, one or no
    friction face active), then fz is raised to fz_min and fx, fy clipped to the box there."""
    a, b, c = v[..., 0], v[..., 1], v[..., 2]
    aa, ab = np.abs(a), np.abs(b)
    lo, hi = np.minimum(aa, ab), np.maximum(aa, ab)
    z_both = (c + mu * (aa + ab)) / (1 + 2 * mu * mu)
    z_one = (c + mu * hi) / (1 + mu * mu)
    fz = np.where(mu * z_both < lo, z_both, np.where(mu * z_one < hi, z_one, c))
    code = (fz < fz_min).astype(np.int64)
    fz = np.maximum(fz, fz_min)
    lim = mu * fz
    code = code | np.where(a > lim, 2, 0) | np.where(a < -lim, 4, 0)
    code = code | np.where(b > lim, 8, 0) | np.where(b < -lim, 16, 0)
    return np.stack([np.clip(a, -lim, lim), np.clip(b, -lim, lim), fz], -1), code


class Problem:
    """The condensed QP of one instance: P (n, n), q (n,), the free-force indices `idx` into the
    force layout [k][leg][axis] (12 N entries), and the rollout map X = G u + c."""

    def __init__(self, inst, Q=Q_DEFAULT, R=R_DEFAULT, mu=0.8, fz_min=10.0):
        Ad, Bd, gd = _f32(inst["Ad"]), _f32(inst["Bd"]), _f32(inst["gd"])
        x0, xref = _f32(inst["x0"]), _f32(inst["xref"])
        ct = np.asarray(inst["contact"]) != 0                        # (4, N)
        N = Bd.shape[0]
        self.N = N
        self.mu, self.fz_min = float(np.float32(mu)), float(np.float32(fz_min))
        self.Q, self.R = _f32(Q), _f32(R)
        self.idx = np.array([12 * k + 3 * l + a for k in range(N) for l in range(4) if ct[l, k]
                             for a in range(3)], int)
        self.n = len(self.idx)
        # x_{k+1} = sum_{j <= k} Ad^(k-j) Bd_j u_j + c_{k+1}
        G = np.zeros((12 * N, 12 * N))
        c = np.zeros((N, 12))
        x = x0
        for k in range(N):
            x = Ad @ x + gd
            c[k] = x
            blk = Bd[k]
            for i in range(k, N):
                G[12 * i:12 * i + 12, 12 * k:12 * k + 12] = blk
                blk = Ad @ blk
        self.G_full, self.c = G, c.reshape(-1)
        self.xref = xref.reshape(-1)
        G = G[:, self.idx]
        Qb = np.tile(self.Q, N)
        Rb = np.tile(self.R, N)[self.idx] if self.n else np.zeros(0)
        self.P = 2.0 * (G.T @ (Qb[:, None] * G) + np.diag(Rb))
        self.q = 2.0 * (G.T @ (Qb * (self.c - self.xref)))

    def full(self, v):
        """Free-force vector(s) (..., n) -> force layout (..., 12 N), swing entries 0."""
        out = np.zeros(v.shape[:-1] + (12 * self.N,))
        out[..., self.idx] = v
        return out

    def states(self, u_full):
        """x_1 .. x_N (12 N,) of a force vector in the force layout."""
        return self.G_full @ u_full + self.c


def run(prob: Problem, max_iter, rho=1e-4, sigma=1e-6, alpha=1.6, adaptive_rho_interval=25,
        eps_abs=1e-4, eps_rel=1e-4):
    """max_iter iterations from the cold start.  Returns a dict of per-iteration arrays (index
    i - 1 for iteration i): z, y, x (max_iter, n), code (max_iter, n / 3), rp, rd, np, nd and rho
    (the rho the iteration ran at), rho_ratio (rho' / rho where an adaptation was decided, else
    NaN), and the exit `status` (2 / -2) with its two ratios `ratio` = (rp / bound, rd / bound)."""
    n = prob.n
    # float32 roundings of the parameters, as the device receives them
    rho0, sigma, alpha = (float(np.float32(v)) for v in (rho, sigma, alpha))
    eps_abs, eps_rel = float(np.float32(eps_abs)), float(np.float32(eps_rel))
    rho = 0.5 * rho0 if n > RHO_LOW_ABOVE else rho0
    x = np.zeros(n); z = np.zeros(n); y = np.zeros(n)
    keys = ("z", "y", "x", "code", "rp", "rd", "np", "nd", "rho", "rho_ratio")
    out = {k: [] for k in keys}
    Pm, q = prob.P, prob.q
    K = None
    for it in range(1, max_iter + 1):
        if K is None:
            K = Pm + (sigma + rho) * np.eye(n)
        g = Pm @ x + q
        xt = np.linalg.solve(K, sigma * x + rho * z - q - y)
        xr = alpha * xt + (1 - alpha) * z
        x = alpha * xt + (1 - alpha) * x
        zt, code = project((xr + y / rho).reshape(-1, 3), prob.mu, prob.fz_min)
        z = zt.reshape(-1)
        y = y + rho * (xr - z)
        rp = np.max(np.abs(x - z))
        rd = np.max(np.abs(g + y))
        npn = max(np.max(np.abs(x)), np.max(np.abs(z)))
        nd = max(np.max(np.abs(g)), np.max(np.abs(y)))
        ratio = np.nan
        rho_it = rho
        if adaptive_rho_interval > 0 and it % adaptive_rho_interval == 0 and it < max_iter:
            new = rho * np.sqrt((rp / npn) / (rd / nd))
            new = min(max(new, 1e-6), 1e6)
            ratio = new / rho
            if new > 5 * rho or new < rho / 5:
                rho = new
                K = None
        for k, v in zip(keys, (z, y, x, code, rp, rd, npn, nd, rho_it, ratio)):
            out[k].append(v)
    out = {k: np.array(v) for k, v in out.items()}
    bp = eps_abs + eps_rel * out["np"][-1]
    bd = eps_abs + eps_rel * out["nd"][-1]
    out["ratio"] = np.array([out["rp"][-1] / bp if bp > 0 else np.inf,
                             out["rd"][-1] / bd if bd > 0 else np.inf])
    out["status"] = 2 if (out["rp"][-1] <= bp and out["rd"][-1] <= bd) else -2
    return out


def instance(batch, i):
    return {k: batch[k][i] for k in ("Ad", "Bd", "gd", "x0", "xref", "contact")}


def problems(batch, **kw):
    return [Problem(instance(batch, i), **kw) for i in range(len(batch["Ad"]))]


def clear_rho(res, margin=1.25):
    """Is every rho decision of a run clear: rho' / rho outside [1 / margin, margin] x each of the
    two thresholds (5 and 1 / 5) at every adaptation?"""
    r = res["rho_ratio"]
    r = r[~np.isnan(r)]
    near = ((r > 5 / margin) & (r < 5 * margin)) | ((r > 0.2 / margin) & (r < 0.2 * margin))
    return not bool(np.any(near))


def clear_status(res, factor=4.0):
    """Are both residual ratios of the exit test a factor >= `factor` away from 1?"""
    r = res["ratio"]
    return bool(np.all((r >= factor) | (r <= 1 / factor)))


def multipliers(prob: Problem, inst, u_full, dtype=np.float64, amb=(1e-7, 1e-4)):
    """include/cmpc.h's lam_out formulas at the force vector u_full (12 N,), in `dtype`
    arithmetic: returns (lam (52 N,), ambiguous (N, 4) bool).  lam_a's dynamics rows are minus the
    adjoint lambda_k of the rollout (lambda_N = 2 Q e_N, lambda_k = 2 Q e_k + Ad' lambda_{k+1});
    with s = 2 R u + Bd_k' lambda_k a swing force has lam_x = -s; a stance leg takes the faces u
    lies on: friction rows max(-+s_x, 0), max(-+s_y, 0), and at fz = fz_min the bound multiplier
    min(-(s_z - mu sum lam_fric), 0).  A face counts as held within 1e-7 relative (of
    max(fz, 1)); a leg whose distance to a face lies between amb[0] and amb[1] relative is
    flagged ambiguous."""
    t = dtype
    N = prob.N
    Ad = np.asarray(inst["Ad"], np.float32).astype(t)
    Bd = np.asarray(inst["Bd"], np.float32).astype(t)
    ct = np.asarray(inst["contact"]) != 0
    Q2, R2 = (2 * prob.Q).astype(t), (2 * prob.R).astype(t)
    mu, fz_min = t(prob.mu), t(prob.fz_min)
    u = np.asarray(u_full).astype(t).reshape(N, 12)
    if t == np.float64:
        e = (prob.states(np.asarray(u_full, np.float64)) - prob.xref).reshape(N, 12)
    else:   # the same rollout carried in `dtype`
        gd = np.asarray(inst["gd"], np.float32); x = np.asarray(inst["x0"], np.float32)
        xr = np.asarray(inst["xref"], np.float32)
        e = np.zeros((N, 12), t)
        for k in range(N):
            x = (Ad @ x + Bd[k] @ u[k] + gd).astype(t)
            e[k] = x - xr[k]
    lam = np.zeros(52 * N, t)
    amb_out = np.zeros((N, 4), bool)
    L = np.zeros(12, t)
    for k in range(N - 1, -1, -1):
        L = (Q2 * e[k] + Ad.T @ L).astype(t)
        lam[24 * N + 12 * k:24 * N + 12 * k + 12] = -L
        s = (R2 * u[k] + Bd[k].T @ L).astype(t)
        for leg in range(4):
            sx, sy, sz = s[3 * leg:3 * leg + 3]
            fx, fy, fz = u[k, 3 * leg:3 * leg + 3]
            lx = lam[12 * N + 12 * k + 3 * leg:12 * N + 12 * k + 3 * leg + 3]
            lf = lam[36 * N + 16 * k + 4 * leg:36 * N + 16 * k + 4 * leg + 4]
            if not ct[leg, k]:
                lx[:] = (-sx, -sy, -sz)
                continue
            sc = max(float(fz), 1.0)
            dist = np.array([fz - fz_min, mu * fz - fx, mu * fz + fx, mu * fz - fy, mu * fz + fy],
                            np.float64) / sc
            amb_out[k, leg] = bool(np.any((dist > amb[0]) & (dist < amb[1])))
            held = dist <= amb[0]
            if held[1]: lf[0] = max(-sx, 0)
            if held[2]: lf[1] = max(sx, 0)
            if held[3]: lf[2] = max(-sy, 0)
            if held[4]: lf[3] = max(sy, 0)
            if held[0]: lx[2] = min(-(sz - mu * lf.sum()), 0)
    return lam, amb_out


def lam_compared(amb):
    """The entries of lam (52 N,) that are compared: all but the bound and friction multipliers
    of the ambiguous legs `amb` (N, 4)."""
    N = amb.shape[0]
    keep = np.ones(52 * N, bool)
    for k, leg in zip(*np.nonzero(amb)):
        keep[12 * N + 12 * k + 3 * leg:12 * N + 12 * k + 3 * leg + 3] = False
        keep[36 * N + 16 * k + 4 * leg:36 * N + 16 * k + 4 * leg + 4] = False
    return keep


# ------------------------------------------------------------------------------------------
# The cases tests/test_admm_ref.py (CPU) and tests/test_gpu_admm_iterates.py (GPU) share
# ------------------------------------------------------------------------------------------
KS = (1, 2, 3, 5, 8, 30)            # max_iter of the iterate runs
KS_OFF = (1, 3, 8)                  # ... at the off-default values
OFF_DEFAULT = (dict(alpha=1.0), dict(alpha=1.9), dict(rho=1e-5), dict(rho=1e-3),
               dict(sigma=0.0), dict(sigma=1e-4))
# Rho adaptation: at the defaults rho' / rho falls through the 1 / 5 threshold smoothly as rp
# shrinks, so most instances take their decision within 25 % of it (tests/test_admm_ref.py prints
# the shares).  From alpha = 1.4, rho = 0.05 the first decision is a clear cut of rho by more
# than 5 / 0.8 on nearly every instance, and the later ones are clear too.
ADAPT = dict(alpha=1.4, rho=0.05)
ADAPT_RUNS = ((2, 8), (2, 9), (3, 8), (3, 9))       # (adaptive_rho_interval, max_iter)
STATUS_RUNS = (dict(max_iter=30), dict(max_iter=27, adaptive_rho_interval=25))
# The status runs use `main` alone: by iteration 27 the step tables at horizons 5 and 1 have
# converged to residuals (1e-10) that a float32 iteration cannot reach.
STATUS_BATCH = "main"
MAX_EXCLUDED = 0.25                 # share of a run's instances that may be unclear

_cache = {}


def bar(k, **params):
    """The GPU bar k iterations after the factorization in use: BAR_FACTOR x D_k (D of the
    largest tabulated k' <= k; the table of D_OFF where `params` holds one of its values)."""
    table = D_K
    for key, t in D_OFF.items():
        if key[0] in params and float(np.float32(params[key[0]])) == float(np.float32(key[1])):
            table = t
    return BAR_FACTOR * table[max(kk for kk in table if kk <= k)]


def since_refactor(res):
    """Iterations a run made at its final rho.  An fp32 x-update's error is (I - M K) x its step;
    it is largest in the first iteration on a new factor (D_1 > D_8) and decays afterwards, so a
    run whose rho changed is held to the bar of the iterations since the change."""
    rho = res["rho"]
    ch = np.flatnonzero(rho[1:] != rho[:-1])
    return len(rho) - (int(ch[-1]) + 1 if len(ch) else 0)


def batches():
    """name -> (N, batch): `main`, test_gpu_admm_passes.batch(16) (n = 24 .. 129, the step tables)
    and two instances each of n = 147, 162, 192 (the NC 160 and NC 192 kernels); `s5` and `s1`,
    the step tables at horizons 5 and 1 (s1's last instance has no stance leg: n = 0)."""
    if "batches" not in _cache:
        from test_gpu_admm_passes import batch, step_batch, KEYS
        from test_gpu_heavy_paths import edge_batch
        m, h = batch(16), edge_batch(per_n=2, targets=(147, 162, 192))
        out = {"main": (16, {k: np.concatenate([m[k], h[k]]) for k in KEYS}),
               "s5": (5, step_batch(5)), "s1": (1, step_batch(1))}
        for _, b in out.values():
            for v in b.values():
                v.setflags(write=False)
        _cache["batches"] = out
    return _cache["batches"]


def batch_problems(name):
    if ("problems", name) not in _cache:
        _cache["problems", name] = problems(batches()[name][1])
    return _cache["problems", name]


def reference(name, max_iter, **params):
    """run() of every instance of batch `name` (None for an instance without a stance leg),
    computed once per parameter set and shared."""
    key = (name, max_iter, tuple(sorted(params.items())))
    if key not in _cache:
        _cache[key] = [run(p, max_iter, **params) if p.n else None for p in batch_problems(name)]
    return _cache[key]


def status_eps(results, rel, factor=4.0):
    """The three tolerances of a status run from its reference residuals (rel: the scaled ones
    rp / np and rd / nd): 4 x the largest, 1 / 4 of the smallest, and one in the middle, with
    the instances whose verdict at the middle one is clear (both residuals a factor >= 4 from it,
    and every rho decision of the run clear).  The middle one is chosen among the geometric
    middles of neighbouring values (all residuals of the batch sorted): the one that leaves the
    fewest instances unclear while both verdicts occur among the clear ones, and of those the one
    in the widest gap.  (The plain geometric middle of the first two tolerances falls among the
    batch's rd values and leaves a third of the instances within a factor 4 of it.)
    Returns (hi, lo, mid, clear (bool per instance), verdict (2 / -2 per instance))."""
    v = np.array([[r["rp"][-1] / (r["np"][-1] if rel else 1.0),
                   r["rd"][-1] / (r["nd"][-1] if rel else 1.0)] for r in results])
    rho_ok = np.array([clear_rho(r) for r in results])
    s = np.sort(v.reshape(-1))
    assert s[0] > 0
    best = None
    for g in range(len(s) - 1):
        mid = float(np.sqrt(s[g] * s[g + 1]))
        clear = np.all((v >= factor * mid) | (v <= mid / factor), axis=1) & rho_ok
        verdict = np.where(np.all(v <= mid, axis=1), 2, -2)
        if set(verdict[clear].tolist()) != {2, -2}:
            continue
        key = (int(np.sum(~clear)), -s[g + 1] / s[g])
        if best is None or key < best[0]:
            best = (key, mid, clear, verdict)
    assert best is not None
    return float(4.0 * s[-1]), float(0.25 * s[0]), best[1], best[2], best[3]
