"""Shared helpers of the cmpc_jvp_run tests (TEST INFRASTRUCTURE, float64 NumPy on the
fp32-rounded arrays the device receives): two independent references of the forward-mode
derivative dw of the optimum on the held faces along a change d_theta of the inputs.

The function differentiated is w*(theta) of include/cmpc.h's cmpc_jvp_io (vjp_util's).

(a) ``ref_dense``: vjp_util._kkt at theta solved by gelsy, K z = rhs; the directional derivative
    of the matrix and of the right-hand side by differencing the assembly itself,
    (_kkt(theta + d) - _kkt(theta - d)) / 2 -- exact, every entry being a polynomial of degree
    <= 2 in theta (``kkt_derivative`` is asserted against the same difference at step 1/2 in
    test_jvp.py) -- and then K dz = d rhs - dK z.  It shares no hand-derived formula with the
    kernel.
(b) ``ref_riccati``: the kernel's route -- gain_util.ref_riccati's recursion (SVD null-space
    basis) for the primal, its rollout, the costates and the face multipliers of a leg by least
    squares (as vjp_util.ref_riccati), then the same recursion with the tangent's linear terms
    as include/cmpc.h lists them, the face offsets by the pseudo-inverse of the leg's rows.

Scale: S_u = max|du_ref| of the instance for the forces; for the states the largest entry of the
tangent rollout with every factor replaced by its absolute value, s_0 = |d_x0|,
s_{k+1} = |Ad| s_k + |Bd_k| |du_k| + |e_k| (dx = sum Bd du cancels where R is small, DESIGN.md
4n).  Entries of du_ref below 1e-11 x max(1e-3 max(|dz|, |d_theta|), max|du|) are set to exactly
zero first, as vjp_util does: S_u = 0 must mean "nothing drives a force".  ``zero_rule``: the force entries the
device gives as exactly 0 -- a swing leg's, and of a leg holding both signs of an axis its fz and
every axis it holds a face of (an axis such a leg holds no face of stays free: the mask rule pins
fz and the held axes only).
"""
from __future__ import annotations

import numpy as np
import scipy.linalg

import vjp_util
from vjp_util import face_rows, _both, _f64
from gain_util import FZ_MIN, FX_POS, FX_NEG, FY_POS, FY_NEG

TANGENTS = vjp_util.OUTPUTS     # ("x0", "xref", "gd", "Q", "R", "mu", "fz_min", "Ad", "Bd")
ORDER = ("Ad", "Bd", "gd", "x0", "xref", "Q", "R", "mu", "fz_min")


def theta_of(Ad, Bd, gd, x0, xref, Q, R, mu, fz_min):
    t = dict(zip(ORDER[:7], _f64(Ad, Bd, gd, x0, xref, Q, R)))
    t["mu"], t["fz_min"] = np.float64(mu), np.float64(fz_min)
    return t


def random_tangents(rng, theta, names=TANGENTS):
    """fp32 tangents of the inputs' shapes: N(0, 1), for mu 0.1 N(0, 1), for R R o N(0, 1) (a
    change of R's own size); theta's values may be batched."""
    out = {}
    for n in names:
        base = np.asarray(theta[n], np.float64)
        v = rng.standard_normal(base.shape)
        if n == "R":
            v = v * base
        if n == "mu":
            v = 0.1 * v
        out[n] = np.asarray(v, np.float32).copy()
    return out


def moved(theta, tangents, h):
    """theta + h d_theta, float64."""
    t = dict(theta)
    for n, d in tangents.items():
        t[n] = np.asarray(theta[n], np.float64) + h * np.asarray(d, np.float64)
    return t


def _kkt_at(t, contact, faces):
    kkt, rhs, n, where = vjp_util._kkt(t["Ad"], t["Bd"], t["gd"], t["x0"], t["xref"], contact,
                                       faces, t["Q"], t["R"], float(t["mu"]), float(t["fz_min"]))
    return kkt, rhs, n


def kkt_derivative(theta, tangents, contact, faces, h=1.0):
    """(dK, d rhs) along the tangents by the central difference of the assembly at step h."""
    Kp, rp, _ = _kkt_at(moved(theta, tangents, h), contact, faces)
    Km, rm, _ = _kkt_at(moved(theta, tangents, -h), contact, faces)
    return (Kp - Km) / (2.0 * h), (rp - rm) / (2.0 * h)


def ref_dense(Ad, Bd, gd, x0, xref, contact, faces, Q, R, mu, fz_min, tangents):
    """Reference (a) -> dw (24N,), states then forces."""
    th = theta_of(Ad, Bd, gd, x0, xref, Q, R, mu, fz_min)
    kkt, rhs, n = _kkt_at(th, contact, faces)
    z = scipy.linalg.lstsq(kkt, rhs, lapack_driver="gelsy")[0]
    dK, drhs = kkt_derivative(th, tangents, contact, faces)
    dz = scipy.linalg.lstsq(kkt, drhs - dK @ z, lapack_driver="gelsy")[0]
    return _snap_forces(dz[:n], max(np.abs(dz).max(), _largest(tangents)))


def _largest(tangents):
    return max(float(np.abs(v).max()) for v in tangents.values())


def _snap_forces(dw, whole):
    dw = np.array(dw, np.float64)
    n = len(dw) // 2
    du = dw[n:]
    du[np.abs(du) <= 1e-11 * max(1e-3 * whole, np.abs(du).max() if du.size else 0.0)] = 0.0
    return dw


def _leg_tangent(mask, mu, fz_min, f, d_mu, d_fz):
    """The held rows A f = b of a stance leg differentiated: -> (A, dA, db - dA f)."""
    A, _, kinds = face_rows(mask, mu, fz_min)
    dA = np.zeros_like(A)
    db = np.zeros(len(A))
    for r, (axis, sign) in enumerate(kinds):
        if axis == "z":
            db[r] = 0.0 if _both(mask) else d_fz
        else:
            dA[r, 2] = -sign * d_mu           # row (1, 0, -sign mu) of a sign-mu face
    return A, dA, db - dA @ f


def ref_riccati(Ad, Bd, gd, x0, xref, contact, faces, Q, R, mu, fz_min, tangents):
    """Reference (b) -> (dw (24N,), info): the kernel's route in NumPy; info holds the primal
    (X, U), the offsets e_k and the scales' ingredients."""
    Ad, Bd, gd, x0, xref, Q, R = _f64(Ad, Bd, gd, x0, xref, Q, R)
    N = Bd.shape[0]
    d = {n: np.asarray(tangents[n], np.float64) if n in tangents else
         np.zeros(np.shape(v)) for n, v in
         dict(x0=x0, xref=xref, gd=gd, Q=Q, R=R, mu=0.0, fz_min=0.0, Ad=Ad, Bd=Bd).items()}
    d_mu, d_fz = float(d["mu"]), float(d["fz_min"])
    Qm, Rm = np.diag(Q), np.diag(R)
    # ---- the primal: recursion, rollout, costates
    P, q = np.zeros((12, 12)), np.zeros(12)
    Ks, ks, Ss, Zs, Gs = [None] * N, [None] * N, [None] * N, [None] * N, [None] * N
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
        S, s = Qm + P, q - Q * xref[k]
        Bt, dd = Bd[k] @ Z, Bd[k] @ c + gd
        if Z.shape[1]:
            G = Bt.T @ S @ Bt + Z.T @ Rm @ Z
            sol = np.linalg.solve(G, np.column_stack([Bt.T @ S @ Ad,
                                                      Bt.T @ (S @ dd + s) + Z.T @ (R * c)]))
            Kk, kk = -Z @ sol[:, :12], c - Z @ sol[:, 12]
        else:
            G, Kk, kk = None, np.zeros((12, 12)), c
        Acl, dcl = Ad + Bd[k] @ Kk, Bd[k] @ kk + gd
        q = Acl.T @ (S @ dcl + s) + Kk.T @ (R * kk)
        P = Acl.T @ S @ Acl + Kk.T @ Rm @ Kk
        P = 0.5 * (P + P.T)
        Ks[k], ks[k], Ss[k], Zs[k], Gs[k] = Kk, kk, S, Z, G
    X, U = np.zeros((N + 1, 12)), np.zeros((N, 12))
    X[0] = x0
    for k in range(N):
        U[k] = Ks[k] @ X[k] + ks[k]
        X[k + 1] = Ad @ X[k] + Bd[k] @ U[k] + gd
    NU = np.zeros((N + 1, 12))
    for k in range(N - 1, -1, -1):
        NU[k] = Ad.T @ NU[k + 1] - 2.0 * Q * (X[k + 1] - xref[k])
    # ---- the tangent's terms, as include/cmpc.h lists them (full scaling: lx' dx + lu' du)
    E = d["gd"] + X[:-1] @ d["Ad"].T + np.einsum("kij,kj->ki", d["Bd"], U)
    lx = 2.0 * (d["Q"] * (X[1:] - xref) - Q * d["xref"]) - NU[1:] @ d["Ad"]
    lu = 2.0 * d["R"] * U - np.einsum("kij,ki->kj", d["Bd"], NU[:-1])
    dC = np.zeros((N, 12))
    for k in range(N):
        rp = 2.0 * R * U[k] - Bd[k].T @ NU[k]
        for leg in range(4):
            sl = slice(3 * leg, 3 * leg + 3)
            mask = int(faces[k, leg]) & 31
            if not contact[leg, k] or not mask:
                continue
            A, dA, rhs = _leg_tangent(mask, mu, fz_min, U[k, sl], d_mu, d_fz)
            dC[k, sl] = np.linalg.lstsq(A, rhs, rcond=None)[0]
            if not _both(mask):                          # dE' nu of the leg's rows
                lu[k, sl] += dA.T @ np.linalg.lstsq(A.T, -rp[sl], rcond=None)[0]
    # ---- the same recursion, the tangent's linear terms
    qa = np.zeros(12)
    kas = [None] * N
    for k in range(N - 1, -1, -1):
        S, Z, c = Ss[k], Zs[k], dC[k]
        sa, r = qa + 0.5 * lx[k], 0.5 * lu[k]
        Bt, dd = Bd[k] @ Z, Bd[k] @ c + E[k]
        if Z.shape[1]:
            ka = c - Z @ np.linalg.solve(Gs[k], Bt.T @ (S @ dd + sa) + Z.T @ (R * c + r))
        else:
            ka = c
        Acl = Ad + Bd[k] @ Ks[k]
        qa = Acl.T @ (S @ (Bd[k] @ ka + E[k]) + sa) + Ks[k].T @ (R * ka + r)
        kas[k] = ka
    floor = max(np.abs(lu).max(), np.abs(lx).max(), _largest(tangents))
    for snap in (False, True):      # again with the forces below the noise floor exactly zero
        dX, dU = np.zeros((N + 1, 12)), np.zeros((N, 12))
        dX[0] = d["x0"]
        for k in range(N):
            dU[k] = Ks[k] @ dX[k] + kas[k]
            if snap:
                dU[k][np.abs(dU[k]) <= cut] = 0.0
            dX[k + 1] = Ad @ dX[k] + Bd[k] @ dU[k] + E[k]
        cut = 1e-11 * max(1e-3 * max(floor, np.abs(dX).max(), np.abs(dU).max()), np.abs(dU).max())
    dw = np.concatenate([dX[1:].ravel(), dU.ravel()])
    return dw, dict(X=X, U=U, E=E, d_x0=d["x0"])


def scales(Ad, Bd, dw_ref, info):
    """(S_x, S_u) of the module's note from a reference dw and ref_riccati's info."""
    Ad, Bd = _f64(Ad, Bd)
    N = Bd.shape[0]
    dU = np.abs(np.asarray(dw_ref, np.float64)[12 * N:].reshape(N, 12))
    s, S_x = np.abs(info["d_x0"]), 0.0
    for k in range(N):
        s = np.abs(Ad) @ s + np.abs(Bd[k]) @ dU[k] + np.abs(info["E"][k])
        S_x = max(S_x, float(s.max()))
    return S_x, float(dU.max()) if dU.size else 0.0


def zero_rule(contact, faces):
    """(N, 12) bool: the force entries that are exactly 0 on the device."""
    N = contact.shape[1]
    z = np.zeros((N, 4, 3), bool)
    for k in range(N):
        for leg in range(4):
            m = int(faces[k, leg]) & 31
            if not contact[leg, k]:
                z[k, leg] = True
            elif _both(m):
                z[k, leg] = [bool(m & (FX_POS | FX_NEG)), bool(m & (FY_POS | FY_NEG)), True]
    return z.reshape(N, 12)


def worst_ratio(got, ref, S_x, S_u, tol):
    """(max |got - ref| / (tol S_x) over the states, the same over the forces with S_u); where a
    scale is 0, 0 if got is exactly zero and the reference below 1e-12, else inf."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    n = len(ref) // 2
    out = []
    for g, r, S in ((got[:n], ref[:n], S_x), (got[n:], ref[n:], S_u)):
        if S > 0.0:
            out.append(float(np.max(np.abs(g - r))) / (tol * S))
        else:
            out.append(0.0 if (np.all(g == 0.0) and np.all(np.abs(r) <= 1e-12)) else np.inf)
    return tuple(out)
