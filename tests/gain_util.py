"""Shared helpers of the cmpc_gain_run tests (TEST INFRASTRUCTURE, float64 NumPy): the face
masks, the per-leg affine set of a mask, and two independent references of the gain K, the
value-function derivatives Vx / Vxx and the optimum u_star on the held faces, both on the
fp32-rounded arrays the device receives.

(a) ``ref_dense``: the face-restricted QP  min 1/2 w'Hw + g'w  s.t.  E w = b(x0)  solved as one
    dense KKT system [[H, E'], [E, 0]] by least squares (E may carry redundant face rows), with
    the extra right-hand-side columns db/dx0: dw/dx0, hence K = d u_0 / d x0,
    Vx = (Hw + g)' dw/dx0 and Vxx = (dw/dx0)' H (dw/dx0).
(b) ``ref_riccati``: the backward Riccati recursion of include/cmpc.h's cmpc_gain_io with an
    orthonormal null-space basis Z from the SVD (not the kernel's Z).

Bar: device and references are float64 and differ in algorithm and summation order; (a) and (b)
agree to ~4e-11 x scale on the fixtures (asserted at 1e-9 in test_gain.py), so the device is held
to TOL_REL = 1e-8 x scale: 250 x that, and below the ~3e-8 floor fp32 data rounding puts on the
forces.  Scale per output: K, max(1, max|K_ref|) of the instance; u_star, max|u_ref| (1 where
the reference has no force at all, ``force_scale``); Vx / Vxx, the largest sum of absolute terms
of the defining product above.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg

TOL_REL = 1e-8
FZ_MIN, FX_POS, FX_NEG, FY_POS, FY_NEG = 1, 2, 4, 8, 16
OUTPUTS = ("K", "Vx", "Vxx", "u_star")


def classify(contact, w, mu, fz_min, tol=1e-6):
    """(N, 4) uint8 masks of the faces w's forces hold: the rule of cmpc.duals.recover (the +
    face of an axis before the - face, threshold tol x max(1, |fz|)); 0 on a swing leg."""
    N = contact.shape[1]
    U = np.asarray(w, np.float64)[12 * N:].reshape(N, 4, 3)
    faces = np.zeros((N, 4), np.uint8)
    for k in range(N):
        for leg in range(4):
            if not contact[leg, k]:
                continue
            fx, fy, fz = U[k, leg]
            scale = tol * max(1.0, abs(fz))
            m = 0
            if abs(fx - mu * fz) <= scale:
                m |= FX_POS
            elif abs(fx + mu * fz) <= scale:
                m |= FX_NEG
            if abs(fy - mu * fz) <= scale:
                m |= FY_POS
            elif abs(fy + mu * fz) <= scale:
                m |= FY_NEG
            if abs(fz - fz_min) <= scale:
                m |= FZ_MIN
            faces[k, leg] = m
    return faces


def threshold_gap(contact, w, mu, fz_min, tol=1e-6):
    """(N, 4) relative distance of the closest face test of each (step, leg) from its threshold
    (inf on a swing leg): where it is tiny, rounding may classify the leg either way."""
    N = contact.shape[1]
    U = np.asarray(w, np.float64)[12 * N:].reshape(N, 4, 3)
    gap = np.full((N, 4), np.inf)
    for k in range(N):
        for leg in range(4):
            if contact[leg, k]:
                fx, fy, fz = U[k, leg]
                t = tol * max(1.0, abs(fz))
                v = np.array([abs(fx - mu * fz), abs(fx + mu * fz), abs(fy - mu * fz),
                              abs(fy + mu * fz), abs(fz - fz_min)])
                gap[k, leg] = np.min(np.abs(v - t)) / t
    return gap


def leg_rows(mask, mu, fz_min):
    """The held faces of a stance leg as equalities A f = b on f = (fx, fy, fz)."""
    A, b = [], []
    if mask & FZ_MIN:
        A.append([0.0, 0.0, 1.0]); b.append(fz_min)
    if mask & FX_POS:
        A.append([1.0, 0.0, -mu]); b.append(0.0)
    if mask & FX_NEG:
        A.append([1.0, 0.0, mu]); b.append(0.0)
    if mask & FY_POS:
        A.append([0.0, 1.0, -mu]); b.append(0.0)
    if mask & FY_NEG:
        A.append([0.0, 1.0, mu]); b.append(0.0)
    return np.array(A, np.float64).reshape(-1, 3), np.array(b, np.float64)


def leg_set_svd(mask, mu, fz_min):
    """-> (Z (3, m) orthonormal null-space basis, c (3,) the least-norm point, consistent)."""
    A, b = leg_rows(mask, mu, fz_min)
    if not len(A):
        return np.eye(3), np.zeros(3), True
    U, s, Vt = np.linalg.svd(A)
    rank = int(np.sum(s > 1e-12 * max(1.0, s[0])))
    c = Vt[:rank].T @ ((U[:, :rank].T @ b) / s[:rank])
    consistent = bool(np.allclose(A @ c, b, rtol=0.0, atol=1e-12 * max(1.0, np.abs(b).max())))
    return Vt[rank:].T.copy(), c, consistent


def leg_set_rule(mask, mu, fz_min):
    """The same set by the mask rule of include/cmpc.h (what the kernel does): both signs of an
    axis held mean fz = 0 and that axis zero; inconsistent only when both signs of an axis come
    with bit 0 and fz_min != 0.  -> (Z (3, m), c (3,), consistent)."""
    pz, xp, xn, yp, yn = (bool(mask & b) for b in (FZ_MIN, FX_POS, FX_NEG, FY_POS, FY_NEG))
    both = (xp and xn) or (yp and yn)
    if both and pz and fz_min != 0.0:
        return np.zeros((3, 0)), np.full(3, np.nan), False
    cols, c = [], np.zeros(3)
    if not (xp or xn):
        cols.append([1.0, 0.0, 0.0])
    if not (yp or yn):
        cols.append([0.0, 1.0, 0.0])
    sx = 0.0 if (xp and xn) or not (xp or xn) else (1.0 if xp else -1.0)
    sy = 0.0 if (yp and yn) or not (yp or yn) else (1.0 if yp else -1.0)
    if pz or both:
        z = 0.0 if both else fz_min
        c = np.array([sx * mu * z, sy * mu * z, z])
    else:
        cols.append([sx * mu, sy * mu, 1.0])
    return np.array(cols, np.float64).reshape(-1, 3).T, c, True


def consistent(faces, contact, mu, fz_min):
    """Every stance mask of the instance is consistent."""
    N = contact.shape[1]
    return all(leg_set_rule(int(faces[k, leg]) & 31, mu, fz_min)[2]
               for k in range(N) for leg in range(4) if contact[leg, k])


def _f64(*a):
    return [np.asarray(x, np.float64) for x in a]


def force_scale(u):
    """max|u|, the scale of u_star -- or 1 where the reference has no force at all (every leg in
    swing or pinned at zero: max|u| is then the solver's noise, ~1e-17, and scales nothing)."""
    m = float(np.abs(u).max())
    return m if m > 1e-9 else 1.0


def ref_dense(Ad, Bd, gd, x0, xref, contact, faces, Q, R, mu, fz_min):
    """Reference (a) -> (vals, S): dicts over OUTPUTS of the values and of the scale of each."""
    Ad, Bd, gd, x0, xref, Q, R = _f64(Ad, Bd, gd, x0, xref, Q, R)
    N = Bd.shape[0]
    n = 24 * N
    H = np.concatenate([np.tile(2.0 * Q, N), np.tile(2.0 * R, N)])
    g = np.concatenate([(-2.0 * Q * xref).reshape(-1), np.zeros(12 * N)])
    rows, b, db = [], [], []
    for k in range(N):                       # x_{k+1} - Ad x_k - Bd_k u_k = gd
        blk = np.zeros((12, n))
        blk[:, 12 * k:12 * k + 12] = np.eye(12)
        if k:
            blk[:, 12 * (k - 1):12 * k] = -Ad
        blk[:, 12 * N + 12 * k:12 * N + 12 * k + 12] = -Bd[k]
        rows.append(blk)
        b.append(gd + (Ad @ x0 if k == 0 else 0.0))
        db.append(Ad if k == 0 else np.zeros((12, 12)))
    for k in range(N):
        for leg in range(4):
            if contact[leg, k]:
                A, rhs = leg_rows(int(faces[k, leg]) & 31, mu, fz_min)
            else:
                A, rhs = np.eye(3), np.zeros(3)
            if len(A):
                blk = np.zeros((len(A), n))
                base = 12 * N + 12 * k + 3 * leg
                blk[:, base:base + 3] = A
                rows.append(blk)
                b.append(rhs)
                db.append(np.zeros((len(A), 12)))
    E, b, db = np.vstack(rows), np.concatenate(b), np.vstack(db)
    m = len(E)
    kkt = np.zeros((n + m, n + m))
    kkt[:n, :n] = np.diag(H)
    kkt[:n, n:] = E.T
    kkt[n:, :n] = E
    rhs = np.zeros((n + m, 13))
    rhs[:n, 0] = -g
    rhs[n:, 0] = b
    rhs[n:, 1:] = db
    # (complete orthogonal factorisation: on these systems closer to (b) than the SVD driver,
    # 2e-12 against 6e-11 x scale, and faster)
    sol = scipy.linalg.lstsq(kkt, rhs, lapack_driver="gelsy")[0]
    w, J = sol[:n, 0], sol[:n, 1:]
    grad = H * w + g
    K = J[12 * N:12 * N + 12]
    vals = dict(K=K, Vx=grad @ J, Vxx=J.T @ (H[:, None] * J), u_star=w[12 * N:])
    S = dict(K=max(1.0, float(np.abs(K).max())), u_star=force_scale(w[12 * N:]),
             Vx=float((np.abs(grad) @ np.abs(J)).max()),
             Vxx=float((np.abs(J).T @ (H[:, None] * np.abs(J))).max()))
    return vals, S


def ref_riccati(Ad, Bd, gd, x0, xref, contact, faces, Q, R, mu, fz_min):
    """Reference (b) -> dict over OUTPUTS: the recursion of cmpc_gain_io, Z from the SVD."""
    Ad, Bd, gd, x0, xref, Q, R = _f64(Ad, Bd, gd, x0, xref, Q, R)
    N = Bd.shape[0]
    Qm, Rm = np.diag(Q), np.diag(R)
    P, q = np.zeros((12, 12)), np.zeros(12)
    Ks, ks = [None] * N, [None] * N
    for k in range(N - 1, -1, -1):
        Z, c = np.zeros((12, 0)), np.zeros(12)
        for leg in range(4):
            if contact[leg, k]:
                Zl, cl, _ = leg_set_svd(int(faces[k, leg]) & 31, mu, fz_min)
                blk = np.zeros((12, Zl.shape[1]))
                blk[3 * leg:3 * leg + 3] = Zl
                Z = np.hstack([Z, blk])
                c[3 * leg:3 * leg + 3] = cl
        S, s = Qm + P, q - Q * xref[k]
        Bt, d = Bd[k] @ Z, Bd[k] @ c + gd
        if Z.shape[1]:
            G = Bt.T @ S @ Bt + Z.T @ Rm @ Z
            sol = np.linalg.solve(G, np.column_stack([Bt.T @ S @ Ad,
                                                      Bt.T @ (S @ d + s) + Z.T @ (R * c)]))
            Kk, kk = -Z @ sol[:, :12], c - Z @ sol[:, 12]
        else:
            Kk, kk = np.zeros((12, 12)), c
        Acl, dcl = Ad + Bd[k] @ Kk, Bd[k] @ kk + gd
        P = Acl.T @ S @ Acl + Kk.T @ Rm @ Kk
        P = 0.5 * (P + P.T)
        q = Acl.T @ (S @ dcl + s) + Kk.T @ (R * kk)
        Ks[k], ks[k] = Kk, kk
    x, U = x0.copy(), np.zeros((N, 12))
    for k in range(N):
        U[k] = Ks[k] @ x + ks[k]
        x = Ad @ x + Bd[k] @ U[k] + gd
    return dict(K=Ks[0], Vx=2.0 * (P @ x0 + q), Vxx=2.0 * P, u_star=U.reshape(-1))


def instance_args(case, i, values):
    """The positional inputs of instance i of a kkt_util-style case, then Q, R, mu, fz_min."""
    return ([case[k][i] for k in ("Ad", "Bd", "gd", "x0", "xref", "contact")],
            dict(Q=values["Q"], R=values["R"], mu=values["mu"], fz_min=values["fz_min"]))


def worst_ratio(dev, vals, S, tol=TOL_REL):
    """max |dev - ref| / (tol x S) per output, over the outputs present in dev."""
    return {n: float(np.max(np.abs(np.asarray(dev[n], np.float64).reshape(np.shape(vals[n])) -
                                   vals[n])) / (tol * S[n])) for n in OUTPUTS if n in dev}
