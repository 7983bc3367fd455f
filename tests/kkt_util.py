"""Shared helpers of the cmpc_kkt_run tests (TEST INFRASTRUCTURE): the float64 NumPy reference
of the four columns and the rounding scale S each column's tolerance is derived from.

Reference: ``oracle.mpc_qp.build_qp`` + ``kkt_residuals`` and ``cmpc.duals.cost`` / ``recover``
on the fp32-rounded arrays the device receives.  Device and reference compute the same float64
function and differ only in the order of their sums, so |dev - ref| <= TOL_REL x S with S the
largest sum of absolute terms in any row of that residual: the longest row has ~30 terms and
the cost 576, so worst-case rounding is ~6e-14 x S.

S per column: cost, the sum of |terms|; stat, max over rows of |H||w| + |g| + |A|'|lam_a| +
|lam_x|; prim, max over rows of |A||w| (|w| for the variable bounds) plus the finite bound; comp,
the same rows times |multiplier|.  With ``lam=None`` the multipliers are the recovered ones.
"""
from __future__ import annotations

import numpy as np

TOL_REL = 1e-12
FIXTURES = (("qp_cfg2.npz", ""), ("qp_terrain.npz", "_A"), ("qp_terrain.npz", "_B"),
            ("qp_weights.npz", "_A"), ("qp_weights.npz", "_B"))


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def plan_constants(params):
    """The plan's Q, R, mu, fz_min as the library holds them: fp32, widened."""
    return dict(Q=f32(params.Q).astype(np.float64), R=f32(params.R).astype(np.float64),
                mu=float(np.float32(params.mu)), fz_min=float(np.float32(params.fz_min)))


def fixture_case(fx, tag, params):
    """One fixture set as the fp32 arrays the device receives: dict with Ad..contact, w, lam
    (B, 52N) and the per-instance mu / fz_min / Q / R the set carries (else absent)."""
    c = {k: f32(fx[k]) for k in ("Ad", "Bd", "gd", "x0", "xref")}
    c["contact"] = np.ascontiguousarray(fx["contact"], dtype=np.uint8)
    c["w"] = f32(fx["w" + tag])
    c["lam"] = f32(np.concatenate([fx["lam_x" + tag], fx["lam_a" + tag]], axis=1))
    for k in ("mu", "fz_min", "Q", "R"):
        if k + tag in fx and tag:
            c[k] = f32(fx[k + tag])
    return c


def instance_values(case, i, params):
    """Q, R (12,), mu, fz_min of instance i in float64: the case's own fp32 entry or the plan's."""
    pc = plan_constants(params)
    out = {}
    for k in ("Q", "R"):
        out[k] = case[k][i].astype(np.float64) if k in case else pc[k]
    for k in ("mu", "fz_min"):
        out[k] = float(case[k][i]) if k in case else pc[k]
    return out


def held_face_tests(contact, w, mu, fz_min, tol=1e-6):
    """(value, threshold) of every held-face test duals.recover can make on w: per stance
    (step, leg) |fx -+ mu fz|, |fy -+ mu fz| and |fz - fz_min| against tol x max(1, |fz|)."""
    N = contact.shape[1]
    U = np.asarray(w, np.float64)[12 * N:].reshape(N, 4, 3)
    vals, thr = [], []
    for k in range(N):
        for leg in range(4):
            if not contact[leg, k]:
                continue
            fx, fy, fz = U[k, leg]
            scale = tol * max(1.0, abs(fz))
            vals += [abs(fx - mu * fz), abs(fx + mu * fz), abs(fy - mu * fz), abs(fy + mu * fz),
                     abs(fz - fz_min)]
            thr += [scale] * 5
    return np.array(vals), np.array(thr)


def kkt_ref(Ad, Bd, gd, x0, xref, contact, w, lam, Q, R, mu, fz_min, tol=1e-6):
    """-> (vals (4,), S (4,)): cost, stat, prim, comp of one instance in float64 NumPy and the
    rounding scale of each.  Inputs are the fp32 arrays (any float dtype, widened here); lam
    (52N,) or None (recovered by cmpc.duals.recover with ``tol``)."""
    from cmpc import duals
    from oracle import mpc_qp
    Ad, Bd, gd, x0, xref, w = (np.asarray(a, np.float64) for a in (Ad, Bd, gd, x0, xref, w))
    Q, R = np.asarray(Q, np.float64), np.asarray(R, np.float64)
    N = Bd.shape[0]
    qp = mpc_qp.build_qp(Ad, Bd, gd, x0, xref.T, contact, Q=Q, R=R, mu=mu, fz_min=fz_min)
    if lam is None:
        lam_x, lam_a = duals.recover(Ad, Bd, gd, x0, xref, contact, w, Q, R, mu, fz_min, tol=tol)
    else:
        lam = np.asarray(lam, np.float64)
        lam_x, lam_a = lam[:24 * N], lam[24 * N:]
    k = mpc_qp.kkt_residuals(qp, w, lam_x, lam_a)
    vals = np.array([duals.cost(w, xref, Q, R), k["stat"], k["prim"], k["comp"]])

    H, A = abs(qp["h"]), abs(qp["a"])
    aw = np.abs(w)
    X, U = aw[:12 * N].reshape(N, 12), aw[12 * N:].reshape(N, 12)
    S_cost = float(np.sum(Q * X * X) + np.sum(R * U * U) + 2.0 * np.sum(Q * np.abs(xref) * X))
    S_stat = float(np.max(H @ aw + np.abs(qp["g"]) + A.T @ np.abs(lam_a) + np.abs(lam_x)))

    def fin(b):
        return np.where(np.isfinite(b), np.abs(b), 0.0)
    row_a = A @ aw + np.maximum(fin(qp["lba"]), fin(qp["uba"]))
    row_x = aw + np.maximum(fin(qp["lbx"]), fin(qp["ubx"]))
    S_prim = float(max(row_a.max(), row_x.max()))
    S_comp = float(max(np.max(np.abs(lam_a) * row_a), np.max(np.abs(lam_x) * row_x)))
    return vals, np.array([S_cost, S_stat, S_prim, S_comp])


def case_ref(case, params, with_lam, tol=1e-6, idx=None):
    """kkt_ref over the instances of a case -> (vals (B, 4), S (B, 4))."""
    B = len(case["w"])
    idx = range(B) if idx is None else idx
    out = [kkt_ref(case["Ad"][i], case["Bd"][i], case["gd"][i], case["x0"][i], case["xref"][i],
                   case["contact"][i], case["w"][i], case["lam"][i] if with_lam else None,
                   tol=tol, **instance_values(case, i, params)) for i in idx]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def assert_matches(dev, vals, S, what=""):
    """Every column of every instance: infinities (and NaNs) in the same places, finite entries
    within TOL_REL x S.  Prints the worst ratio per column before asserting."""
    dev, vals = np.asarray(dev, np.float64), np.asarray(vals, np.float64)
    assert dev.shape == vals.shape, (dev.shape, vals.shape)
    finite = np.isfinite(vals)
    err = np.where(finite, np.abs(np.where(finite, dev, 0.0) - np.where(finite, vals, 0.0)), 0.0)
    ratio = err / np.maximum(TOL_REL * S, np.finfo(np.float64).tiny)
    print(what, "worst |dev - ref| / (1e-12 S) per column:", ratio.max(axis=0),
          "inf comp:", int(np.isinf(vals[:, 3]).sum()), "of", len(vals))
    assert np.array_equal(np.isfinite(dev), finite), \
        (what, np.argwhere(np.isfinite(dev) != finite)[:8])
    assert np.array_equal(dev[~finite], vals[~finite], equal_nan=True), what
    assert np.all(err <= TOL_REL * S), (what, np.argwhere(err > TOL_REL * S)[:8], ratio.max(axis=0))
