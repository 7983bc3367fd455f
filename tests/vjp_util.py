"""Shared helpers of the cmpc_vjp_run tests (TEST INFRASTRUCTURE, float64 NumPy on the
fp32-rounded arrays the device receives): two independent references of the gradients of a loss
through the optimum on the held faces, and the central-difference function they are checked
against.

The function differentiated is w*(theta) of include/cmpc.h's cmpc_vjp_io: the minimiser of
1/2 w'Hw + g'w over the dynamics and the held faces, the face set fixed (gain_util's u_star and
its rollout).  With [[H, E'], [E, 0]] [dw; dnu] = [-gw; 0] every gradient is a product of
(w, nu) with (dw, dnu); ``assemble`` holds those formulas once for both references.

(a) ``ref_dense``: the dense KKT system by complete orthogonal factorisation (gelsy), with the
    right-hand sides [-g; b] and [-gw; 0].
(b) ``ref_riccati``: the kernel's route -- gain_util.ref_riccati's recursion (SVD null-space
    basis) with the adjoint's linear terms next to the primal ones, a forward pass, the backward
    costate pass, and the face multipliers of a leg by least squares on its stationarity residual.

A leg that holds both signs of an axis is pinned at fz = 0 whatever mu and fz_min are (the mask
rule of cmpc_gain_io), so it contributes nothing to g_mu and g_fz_min; its face rows enter E with
a zero right-hand side.

Scale S per output: the defining formula with every factor replaced by its absolute value, the
largest entry.  Both references first set entries of (dx, du) and of u below 1e-11 x the largest
of their vector to exactly zero (the largest: at least 1 for u and 1e-3 max|gw| for the adjoint in
(b); at least 1e-3 x the largest entry of the whole solution, multipliers included, in (a), whose
noise is relative to that): a force that is pinned, or an adjoint that nothing drives, is
zero by construction on the device, but 1e-17 out of a dense solve or an SVD basis, and S = 0
must mean "every term has a factor that is exactly zero".
"""
from __future__ import annotations

import numpy as np
import scipy.linalg

import gain_util
from gain_util import FZ_MIN, FX_POS, FX_NEG, FY_POS, FY_NEG

TOL_REL = 1e-8      # device against either reference, x S (gain_util's bar)
TOL_REFS = 1e-9     # (a) against (b), x S (test_gain.py's bar for its two references)
OUTPUTS = ("x0", "xref", "gd", "Q", "R", "mu", "fz_min", "Ad", "Bd")


def shapes(B, N):
    return dict(x0=(B, 12), xref=(B, N, 12), gd=(B, 12), Q=(B, 12), R=(B, 12), mu=(B,),
                fz_min=(B,), Ad=(B, 12, 12), Bd=(B, N, 12, 12))


def _f64(*a):
    return [np.asarray(x, np.float64) for x in a]


def _both(mask):
    return (mask & 6) == 6 or (mask & 24) == 24


def face_rows(mask, mu, fz_min):
    """gain_util.leg_rows with the mask rule's right-hand side: both signs of an axis pin fz = 0.
    -> (A (m, 3), b (m,), kinds): kinds[r] = ("z", 0) or ("x" | "y", +1 | -1) for a +mu | -mu face."""
    A, b = gain_util.leg_rows(mask, mu, fz_min)
    kinds = [k for bit, k in ((FZ_MIN, ("z", 0)), (FX_POS, ("x", 1)), (FX_NEG, ("x", -1)),
                              (FY_POS, ("y", 1)), (FY_NEG, ("y", -1))) if mask & bit]
    if _both(mask):
        b = np.zeros_like(b)
    return A, b, kinds


def _snap(v, floor):
    v = np.array(v, np.float64)
    m = max(np.abs(v).max() if v.size else 0.0, floor)
    v[np.abs(v) <= 1e-11 * m] = 0.0
    return v


def assemble(Ad, Bd, xref, Q, mu, X, U, dX, dU, NU, dNU, face_mult):
    """The outputs and their scales from the primal (X (N+1, 12) = x_0..x_N, U, NU) and adjoint
    (dX, dU, dNU) solutions and ``face_mult``: (k, leg, kind, nu_r, dnu_r) of every held face row
    of a stance leg that does not hold both signs of an axis."""
    N = len(U)
    a = np.abs
    ex = X[1:] - xref
    vals = dict(x0=-Ad.T @ dNU[0], xref=-2.0 * Q * dX[1:], gd=-dNU.sum(axis=0),
                Q=2.0 * np.sum(dX[1:] * ex, axis=0), R=2.0 * np.sum(dU * U, axis=0),
                Ad=-(NU.T @ dX[:-1] + dNU.T @ X[:-1]),
                Bd=-(NU[:, :, None] * dU[:, None, :] + dNU[:, :, None] * U[:, None, :]))
    S = dict(x0=a(Ad).T @ a(dNU[0]), xref=2.0 * Q * a(dX[1:]), gd=a(dNU).sum(axis=0),
             Q=2.0 * np.sum(a(dX[1:]) * a(ex), axis=0), R=2.0 * np.sum(a(dU) * a(U), axis=0),
             Ad=a(NU).T @ a(dX[:-1]) + a(dNU).T @ a(X[:-1]),
             Bd=a(NU)[:, :, None] * a(dU)[:, None, :] + a(dNU)[:, :, None] * a(U)[:, None, :])
    g_mu = g_fz = s_mu = s_fz = 0.0
    for k, leg, (axis, sign), nu_r, dnu_r in face_mult:
        if axis == "z":
            g_fz -= dnu_r
            s_fz += abs(dnu_r)
        else:
            fz, dfz = U[k, 3 * leg + 2], dU[k, 3 * leg + 2]
            g_mu -= sign * (nu_r * dfz + dnu_r * fz)
            s_mu += abs(nu_r * dfz) + abs(dnu_r * fz)
    vals.update(mu=np.float64(g_mu), fz_min=np.float64(g_fz))
    S.update(mu=s_mu, fz_min=s_fz)
    return vals, {n: float(np.max(v)) for n, v in S.items()}


def _kkt(Ad, Bd, gd, x0, xref, contact, faces, Q, R, mu, fz_min):
    """-> (kkt matrix, [-g; b], n, row index: ("dyn", k) -> slice, (k, leg) -> (slice, kinds))."""
    N = Bd.shape[0]
    n = 24 * N
    H = np.concatenate([np.tile(2.0 * Q, N), np.tile(2.0 * R, N)])
    g = np.concatenate([(-2.0 * Q * xref).reshape(-1), np.zeros(12 * N)])
    rows, b, where, at = [], [], {}, 0
    for k in range(N):
        blk = np.zeros((12, n))
        blk[:, 12 * k:12 * k + 12] = np.eye(12)
        if k:
            blk[:, 12 * (k - 1):12 * k] = -Ad
        blk[:, 12 * N + 12 * k:12 * N + 12 * k + 12] = -Bd[k]
        rows.append(blk)
        b.append(gd + (Ad @ x0 if k == 0 else 0.0))
        at += 12
    for k in range(N):
        for leg in range(4):
            if contact[leg, k]:
                A, rhs, kinds = face_rows(int(faces[k, leg]) & 31, mu, fz_min)
            else:
                A, rhs, kinds = np.eye(3), np.zeros(3), None
            if len(A):
                blk = np.zeros((len(A), n))
                base = 12 * N + 12 * k + 3 * leg
                blk[:, base:base + 3] = A
                rows.append(blk)
                b.append(rhs)
                if kinds is not None and not _both(int(faces[k, leg]) & 31):
                    where[(k, leg)] = (slice(at, at + len(A)), kinds)
                at += len(A)
    E, b = np.vstack(rows), np.concatenate(b)
    m = len(E)
    kkt = np.zeros((n + m, n + m))
    kkt[:n, :n] = np.diag(H)
    kkt[:n, n:] = E.T
    kkt[n:, :n] = E
    return kkt, np.concatenate([-g, b]), n, where


def w_star(Ad, Bd, gd, x0, xref, contact, faces, Q, R, mu, fz_min):
    """The optimum on the held faces (24N,), states then forces: what central differences move."""
    Ad, Bd, gd, x0, xref, Q, R = _f64(Ad, Bd, gd, x0, xref, Q, R)
    kkt, rhs, n, _ = _kkt(Ad, Bd, gd, x0, xref, contact, faces, Q, R, float(mu), float(fz_min))
    return scipy.linalg.lstsq(kkt, rhs, lapack_driver="gelsy")[0][:n]


def ref_dense(Ad, Bd, gd, x0, xref, contact, faces, Q, R, mu, fz_min, gw):
    """Reference (a) -> (vals, S): dicts over OUTPUTS."""
    Ad, Bd, gd, x0, xref, Q, R, gw = _f64(Ad, Bd, gd, x0, xref, Q, R, gw)
    N = Bd.shape[0]
    kkt, rhs, n, where = _kkt(Ad, Bd, gd, x0, xref, contact, faces, Q, R, mu, fz_min)
    rhs2 = np.zeros((len(rhs), 2))
    rhs2[:, 0] = rhs
    rhs2[:n, 1] = -gw
    sol = scipy.linalg.lstsq(kkt, rhs2, lapack_driver="gelsy")[0]
    w, dw, nu, dnu = sol[:n, 0], sol[:n, 1], sol[n:, 0], sol[n:, 1]
    X = np.vstack([x0, w[:12 * N].reshape(N, 12)])
    dX = np.vstack([np.zeros(12), dw[:12 * N].reshape(N, 12)])
    U = _snap(w[12 * N:], max(1.0, 1e-3 * np.abs(sol[:, 0]).max())).reshape(N, 12)
    dU = dw[12 * N:].reshape(N, 12)
    dall = _snap(np.concatenate([dX.ravel(), dU.ravel()]), 1e-3 * np.abs(sol[:, 1]).max())
    dX, dU = dall[:12 * (N + 1)].reshape(N + 1, 12), dall[12 * (N + 1):].reshape(N, 12)
    fm = [(k, leg, kind, nu[sl][r], dnu[sl][r]) for (k, leg), (sl, kinds) in where.items()
          for r, kind in enumerate(kinds)]
    return assemble(Ad, Bd, xref, Q, mu, X, U, dX, dU, nu[:12 * N].reshape(N, 12),
                    dnu[:12 * N].reshape(N, 12), fm)


def ref_riccati(Ad, Bd, gd, x0, xref, contact, faces, Q, R, mu, fz_min, gw):
    """Reference (b) -> (vals, S): the kernel's route in NumPy."""
    Ad, Bd, gd, x0, xref, Q, R, gw = _f64(Ad, Bd, gd, x0, xref, Q, R, gw)
    N = Bd.shape[0]
    gx, gu = gw[:12 * N].reshape(N, 12), gw[12 * N:].reshape(N, 12)
    Qm, Rm = np.diag(Q), np.diag(R)
    P, q, qa = np.zeros((12, 12)), np.zeros(12), np.zeros(12)
    Ks, ks, kas = [None] * N, [None] * N, [None] * N
    for k in range(N - 1, -1, -1):
        Z, c = np.zeros((12, 0)), np.zeros(12)
        for leg in range(4):
            if contact[leg, k]:
                A, rhs, _ = face_rows(int(faces[k, leg]) & 31, mu, fz_min)
                if len(A):
                    Uu, s_, Vt = np.linalg.svd(A)
                    rank = int(np.sum(s_ > 1e-12 * max(1.0, s_[0])))
                    Zl = Vt[rank:].T
                    cl = Vt[:rank].T @ ((Uu[:, :rank].T @ rhs) / s_[:rank])
                else:
                    Zl, cl = np.eye(3), np.zeros(3)
                blk = np.zeros((12, Zl.shape[1]))
                blk[3 * leg:3 * leg + 3] = Zl
                Z = np.hstack([Z, blk])
                c[3 * leg:3 * leg + 3] = cl
        S, s, sa, r = Qm + P, q - Q * xref[k], qa + 0.5 * gx[k], 0.5 * gu[k]
        Bt, d = Bd[k] @ Z, Bd[k] @ c + gd
        if Z.shape[1]:
            G = Bt.T @ S @ Bt + Z.T @ Rm @ Z
            sol = np.linalg.solve(G, np.column_stack([Bt.T @ S @ Ad,
                                                      Bt.T @ (S @ d + s) + Z.T @ (R * c),
                                                      Bt.T @ sa + Z.T @ r]))
            Kk, kk, ka = -Z @ sol[:, :12], c - Z @ sol[:, 12], -Z @ sol[:, 13]
        else:
            Kk, kk, ka = np.zeros((12, 12)), c, np.zeros(12)
        Acl, dcl, dca = Ad + Bd[k] @ Kk, Bd[k] @ kk + gd, Bd[k] @ ka
        q = Acl.T @ (S @ dcl + s) + Kk.T @ (R * kk)
        qa = Acl.T @ (S @ dca + sa) + Kk.T @ (R * ka + r)
        P = Acl.T @ S @ Acl + Kk.T @ Rm @ Kk
        P = 0.5 * (P + P.T)
        Ks[k], ks[k], kas[k] = Kk, kk, ka
    X, dX = np.zeros((N + 1, 12)), np.zeros((N + 1, 12))
    U, dU = np.zeros((N, 12)), np.zeros((N, 12))
    X[0] = x0
    for k in range(N):
        U[k] = Ks[k] @ X[k] + ks[k]
        dU[k] = Ks[k] @ dX[k] + kas[k]
        X[k + 1] = Ad @ X[k] + Bd[k] @ U[k] + gd
        dX[k + 1] = Ad @ dX[k] + Bd[k] @ dU[k]
    U = _snap(U.ravel(), 1.0).reshape(N, 12)
    dall = _snap(np.concatenate([dX.ravel(), dU.ravel()]), 1e-3 * np.abs(gw).max())
    dX, dU = dall[:12 * (N + 1)].reshape(N + 1, 12), dall[12 * (N + 1):].reshape(N, 12)
    NU, dNU = np.zeros((N, 12)), np.zeros((N, 12))
    nxt, dnxt = np.zeros(12), np.zeros(12)
    for k in range(N - 1, -1, -1):
        NU[k] = nxt = Ad.T @ nxt - 2.0 * Q * (X[k + 1] - xref[k])
        dNU[k] = dnxt = Ad.T @ dnxt - 2.0 * Q * dX[k + 1] - gx[k]
    fm = []
    for k in range(N):
        rp = 2.0 * R * U[k] - Bd[k].T @ NU[k]
        ra = 2.0 * R * dU[k] + gu[k] - Bd[k].T @ dNU[k]
        for leg in range(4):
            mask = int(faces[k, leg]) & 31
            if not contact[leg, k] or _both(mask):
                continue
            A, _, kinds = face_rows(mask, mu, fz_min)
            if len(A):
                sl = slice(3 * leg, 3 * leg + 3)
                m_p = np.linalg.lstsq(A.T, -rp[sl], rcond=None)[0]
                m_a = np.linalg.lstsq(A.T, -ra[sl], rcond=None)[0]
                fm += [(k, leg, kind, m_p[r_], m_a[r_]) for r_, kind in enumerate(kinds)]
    return assemble(Ad, Bd, xref, Q, mu, X, U, dX, dU, NU, dNU, fm)


def worst_ratio(got, vals, S, tol):
    """max |got - ref| / (tol x S) per output present in got; where S is 0, 0 if got is exactly
    zero and the reference below 1e-12, else inf."""
    out = {}
    for n in OUTPUTS:
        if n not in got:
            continue
        g = np.asarray(got[n], np.float64).reshape(np.shape(vals[n]))
        err = float(np.max(np.abs(g - vals[n])))
        if S[n] > 0.0:
            out[n] = err / (tol * S[n])
        else:
            out[n] = 0.0 if (np.all(g == 0.0) and np.all(np.abs(vals[n]) <= 1e-12)) else np.inf
    return out


def random_gw(rng, shape):
    """dL/dw ~ N(0, 1), rounded to fp32."""
    return np.ascontiguousarray(rng.standard_normal(shape).astype(np.float32))
