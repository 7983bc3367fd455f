"""Shared helpers of the cmpc_refine_run tests (TEST INFRASTRUCTURE, float64 NumPy): the model of
the certified refinement of include/cmpc.h's cmpc_refine_io, decision by decision, built on
``gain_util.ref_riccati`` (the optimum on the held faces, Z from the SVD, not the kernel's Z).

Per round: (u, x) the optimum on the held faces and its rollout; the costate pass
p_k = 2Q (x_{k+1} - xref_k) + Ad' p_{k+1}; g_k = 2R u_k + Bd_k' p_k; per stance leg the multipliers
lam_x = -sx gx, lam_y = -sy gy of the held friction faces and lam_z = gz - mu (lam_x + lam_y) of a
held fz face; with us = max(1, max|u|), gs = us min 2R: a face not held is violated when its row
(fz_min - fz, fx - mu fz, -fx - mu fz, fy - mu fz, -fy - mu fz) is above prim_tol us (of two
violated signs of an axis only the larger row, the + face on a tie), a held face negative when
its multiplier is below -dual_tol gs.  Neither: certified.  r == max_rounds: ROUNDS.  Violated
faces are all added (the other sign of the axis cleared) and nothing dropped; with none violated
every negative face is dropped.  New masks equal to an earlier round's: CYCLE.

Bars.
* Device against model: both are float64 and differ in algorithm (the kernel's Z against the
  SVD's) and summation order, so the forces are held to ``gain_util.TOL_REL`` (1e-8) x the force
  scale max|u|, the project's bar for this recursion.  The states inherit it through the rollout
  (x the largest |dx/du| row sum, taken as the state scale max(1, max|x|)); the multipliers are
  sums of 2R u and Bd' p terms, lam_z of up to three entries of g (mu <= 1), and are held to
  1e-8 x 3 x the largest sum of absolute terms of an entry of g (``lam_scale``); res[0] (a
  difference of two forces, mu <= 1) and res[1] are those quantities divided by us and gs.
* Model against oracle (``oracle.active_set.certified_optimum`` on the same fp32-widened
  inputs): measured at 1.4e-13 x max|u| on qp_cfg2, asserted at ORACLE_REL = 1e-10.
* A decision is "clear" when every tested quantity of every round is a factor CLEAR = 2 away from
  its threshold (``margin`` >= 2): 1e-8-relative differences cannot flip a clear decision, and
  info / faces are compared exactly only there.
"""
from __future__ import annotations

import numpy as np

import gain_util

INVALID, ROUNDS, CYCLE = -1, -2, -3
ORACLE_REL = 1e-10
CLEAR = 2.0
BITS = (gain_util.FZ_MIN, gain_util.FX_POS, gain_util.FX_NEG, gain_util.FY_POS, gain_util.FY_NEG)


def _clearance(q, t):
    """How far the test q > t (t > 0) is from flipping: max(q / t, t / q), inf for q <= 0."""
    return np.inf if q <= 0.0 else max(q / t, t / q)


def model(Ad, Bd, gd, x0, xref, contact, faces, Q, R, mu, fz_min, u_in=None, max_rounds=8,
          prim_tol=1e-9, dual_tol=1e-9):
    """One instance -> dict(info, faces (N, 4) uint8, u (12N,), x (N, 12) = x_1..x_N, lam (52N,)
    = [lam_x | lam_a] in cmpc.duals.recover's layout, res (3,), margin, lam_scale).  ``faces``
    (N, 4) masks; ``u_in`` (12N,) the forces res[2] is measured from (None: NaN)."""
    Ad, Bd, gd, x0, xref, Q, R = (np.asarray(a, np.float64) for a in (Ad, Bd, gd, x0, xref, Q, R))
    N = Bd.shape[0]
    stance = contact.T != 0
    masks = np.where(stance, np.asarray(faces) & 31, 0).astype(np.uint8)
    apex = ((masks & 6) == 6) | ((masks & 24) == 24)
    valid = (np.all(np.isfinite(Q)) and np.all(Q >= 0) and np.all(np.isfinite(R)) and
             np.all(R > 0) and np.isfinite(mu) and mu > 0 and np.isfinite(fz_min))
    if not valid or apex.any():
        return dict(info=INVALID, faces=np.full((N, 4), 0xFF, np.uint8), u=np.full(12 * N, np.nan),
                    x=np.full((N, 12), np.nan), lam=np.full(52 * N, np.nan),
                    res=np.full(3, np.nan), margin=np.inf, lam_scale=1.0)
    hist, margin, r = [], np.inf, 0
    while True:
        hist.append(masks.copy())
        u = gain_util.ref_riccati(Ad, Bd, gd, x0, xref, contact, masks, Q, R, mu,
                                  fz_min)["u_star"].reshape(N, 12)
        X = np.zeros((N + 1, 12))
        X[0] = x0
        for k in range(N):
            X[k + 1] = Ad @ X[k] + Bd[k] @ u[k] + gd
        P = np.zeros((N + 1, 12))
        for k in range(N - 1, -1, -1):
            P[k] = 2.0 * Q * (X[k + 1] - xref[k]) + Ad.T @ P[k + 1]
        g = np.stack([2.0 * R * u[k] + Bd[k].T @ P[k] for k in range(N)])
        lam_scale = 3.0 * max(float(np.max(2.0 * R * np.abs(u[k]) + np.abs(Bd[k]).T @ np.abs(P[k])))
                              for k in range(N))
        us = max(1.0, float(np.abs(u).max()))
        gs = us * float(np.min(2.0 * R))
        lam = np.zeros((N, 4, 5))          # per leg in BITS order: fz, x+, x-, y+, y-
        viol = np.zeros((N, 4), np.uint8)
        neg = np.zeros((N, 4), np.uint8)
        vmax, lmin = 0.0, 0.0
        for k in range(N):
            for leg in range(4):
                if not stance[k, leg]:
                    continue
                m = int(masks[k, leg])
                fx, fy, fz = u[k, 3 * leg:3 * leg + 3]
                gx, gy, gz = g[k, 3 * leg:3 * leg + 3]
                l = lam[k, leg]
                if m & 2:
                    l[1] = -gx
                if m & 4:
                    l[2] = gx
                if m & 8:
                    l[3] = -gy
                if m & 16:
                    l[4] = gy
                if m & 1:
                    l[0] = gz - mu * (l[1] + l[2] + l[3] + l[4])
                v = np.array([fz_min - fz, fx - mu * fz, -fx - mu * fz, fy - mu * fz, -fy - mu * fz])
                vb = 0
                for i, bit in enumerate(BITS):
                    if m & bit:
                        lmin = min(lmin, l[i])
                        margin = min(margin, _clearance(-l[i], dual_tol * gs))
                        if l[i] < -dual_tol * gs:
                            neg[k, leg] |= bit
                    else:
                        vmax = max(vmax, v[i])
                        margin = min(margin, _clearance(v[i], prim_tol * us))
                        if v[i] > prim_tol * us:
                            vb |= bit
                for a, b, ia, ib in ((2, 4, 1, 2), (8, 16, 3, 4)):
                    if vb & a and vb & b:          # both signs violated: the larger row counts
                        margin = min(margin, _clearance(abs(v[ia] - v[ib]), prim_tol * us))
                        vb &= ~b if v[ia] >= v[ib] else ~a
                viol[k, leg] = vb
        if not viol.any() and not neg.any():
            info = r
            break
        if r == max_rounds:
            info = ROUNDS
            break
        if viol.any():
            nxt = masks | viol
            nxt = np.where(viol & 2, nxt & ~np.uint8(4), nxt)
            nxt = np.where(viol & 4, nxt & ~np.uint8(2), nxt)
            nxt = np.where(viol & 8, nxt & ~np.uint8(16), nxt)
            nxt = np.where(viol & 16, nxt & ~np.uint8(8), nxt).astype(np.uint8)
        else:
            nxt = (masks & ~neg).astype(np.uint8)
        if any(np.array_equal(nxt, h) for h in hist):
            info = CYCLE
            break
        masks, r = nxt, r + 1
    lam_x = np.zeros(24 * N)
    lam_fric = np.zeros((N, 4, 4))
    for k in range(N):
        for leg in range(4):
            base = 12 * N + 12 * k + 3 * leg
            if stance[k, leg]:
                lam_x[base + 2] = -lam[k, leg, 0]
                lam_fric[k, leg] = lam[k, leg, 1:]
            else:
                lam_x[base:base + 3] = -g[k, 3 * leg:3 * leg + 3]
    res2 = np.nan
    if u_in is not None:
        u_in = np.asarray(u_in, np.float64).reshape(-1)
        res2 = float(np.abs(u.reshape(-1) - u_in).max() / max(1.0, np.abs(u_in).max()))
    return dict(info=info, faces=masks, u=u.reshape(-1), x=X[1:],
                lam=np.concatenate([lam_x, -P[:N].reshape(-1), lam_fric.reshape(-1)]),
                res=np.array([vmax / us, lmin / gs, res2]), margin=margin, lam_scale=lam_scale)


def model_case(case, i, params, faces=None, tol=1e-6, **kw):
    """The model on instance i of a kkt_util-style case: faces given (N, 4), or read off the
    case's w by the face rule with ``tol``; u_in = w's forces where the case has a w."""
    import kkt_util
    iv = kkt_util.instance_values(case, i, params)
    args, vals = gain_util.instance_args(case, i, iv)
    N = case["Bd"].shape[1]
    if faces is None:
        faces = gain_util.classify(case["contact"][i], case["w"][i], iv["mu"], iv["fz_min"], tol)
    u_in = case["w"][i][12 * N:] if "w" in case else None
    return model(*args, faces, vals["Q"], vals["R"], vals["mu"], vals["fz_min"], u_in=u_in, **kw)


def oracle_optimum(case, i, params, seed):
    """oracle.active_set.certified_optimum of instance i on the fp32-widened inputs, seeded by
    ``seed`` (24N,) -> its result dict, with the qp under "qp"."""
    import kkt_util
    from oracle import active_set, mpc_qp
    iv = kkt_util.instance_values(case, i, params)
    f64 = [np.asarray(case[k][i], np.float64) for k in ("Ad", "Bd", "gd", "x0", "xref")]
    qp = mpc_qp.build_qp(f64[0], f64[1], f64[2], f64[3], f64[4].T, case["contact"][i], Q=iv["Q"],
                         R=iv["R"], mu=iv["mu"], fz_min=iv["fz_min"])
    r = active_set.certified_optimum(qp, np.asarray(seed, np.float64))
    r["qp"] = qp
    return r


def wrong_face_seeds(faces, contact, recipe, seed=7):
    """One wrong face per instance, chosen by default_rng(seed): recipe "drop" clears one held
    face of a stance leg, "add" sets one face of a stance leg that holds none on that axis.
    faces (B, N, 4), contact (B, 4, N) -> a copy with the change (an instance without a
    candidate is left as it is)."""
    rng = np.random.default_rng(seed)
    out = faces.copy()
    for b in range(len(faces)):
        stance = contact[b].T != 0
        cand = []
        for k, leg in zip(*np.nonzero(stance)):
            m = int(faces[b, k, leg])
            if recipe == "drop":
                cand += [(k, leg, bit) for bit in BITS if m & bit]
            else:
                if not m & 1:
                    cand.append((k, leg, 1))
                if not m & 6:
                    cand += [(k, leg, 2), (k, leg, 4)]
                if not m & 24:
                    cand += [(k, leg, 8), (k, leg, 16)]
        if cand:
            k, leg, bit = cand[int(rng.integers(len(cand)))]
            out[b, k, leg] ^= bit
    return out
