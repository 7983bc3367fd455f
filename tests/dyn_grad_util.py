"""Shared helpers of the cmpc_dynamics_vjp_run / cmpc_dynamics_jvp_run tests (TEST INFRASTRUCTURE,
float64 NumPy on the fp32-rounded inputs, dt included, that the device receives): the closed form
of the dynamics builder, its reverse- and forward-mode derivatives written out from the formulas
of include/cmpc.h with einsum over the whole batch, and the scale S of every output.

Per robot, with h2 = dt^2/2:  minv = 1/m,  J = inertia^-1 (nine independent entries),
yaw = mean_k xref[k][5],  Rt = [[c, s, 0], [-s, c, 0], [0, 0, 1]];  per (step k, leg l)
S = [r_kl]x,  W = J S,  V = Rt W, and the blocks of Bd_k[:, 3l:3l+3] are h2 minv I3, h2 V,
dt minv I3, dt W;  Ad[3:6, 9:12] = dt Rt.

Scale S per output and robot: the defining formula with every factor replaced by its absolute
value, through the intermediates as well (|J|, |S|, |M|, |W|, ..), the largest entry of the
robot's part of that output.  In g_yaw each of the four terms carries |c| + |s|: an error of the
mean yaw moves c by s and s by c, so a term's error is not bounded by its own factor alone.
"""
from __future__ import annotations

import numpy as np

VJP_OUTPUTS = ("mass", "inertia", "r_feet", "yaw")
JVP_TANGENTS = ("mass", "inertia", "r_feet", "xref")
JVP_OUTPUTS = ("Ad", "Bd")
TOL = 1e-12         # device against the reference, x S (the issue's derivation: ~2e-14 x S expected)
REL32 = 2.0 ** -23  # one fp32 rounding of the jvp's outputs


def f32(a):
    """The array as the device receives it: rounded to fp32, widened exactly."""
    return np.asarray(np.asarray(a, np.float32), np.float64)


def skew(r):
    """[r]x of (..., 3) -> (..., 3, 3)."""
    S = np.zeros(r.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2] = -r[..., 2], r[..., 1]
    S[..., 1, 0], S[..., 1, 2] = r[..., 2], -r[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -r[..., 1], r[..., 0]
    return S


def unskew(G):
    """The gradient in r of a gradient G in [r]x: (..., 3, 3) -> (..., 3)."""
    return np.stack([G[..., 2, 1] - G[..., 1, 2], G[..., 0, 2] - G[..., 2, 0],
                     G[..., 1, 0] - G[..., 0, 1]], axis=-1)


def _robot(mass, inertia, xref):
    """-> minv (B,), J (B,3,3), c, s (B,), Rt (B,3,3)."""
    minv = 1.0 / mass
    J = np.linalg.inv(inertia)
    yaw = xref[:, :, 5].sum(axis=1) / xref.shape[1]
    c, s = np.cos(yaw), np.sin(yaw)
    Rt = np.zeros((len(mass), 3, 3))
    Rt[:, 0, 0], Rt[:, 0, 1], Rt[:, 1, 0], Rt[:, 1, 1], Rt[:, 2, 2] = c, s, -s, c, 1.0
    return minv, J, c, s, Rt


def _blocks(B, N, b0, b1, b2, b3):
    """(B, N, 12, 12) from the four (B, N, 4, 3, 3) row groups of every leg's column block."""
    out = np.zeros((B, N, 12, 12))
    for l in range(4):
        for q, blk in enumerate((b0, b1, b2, b3)):
            out[:, :, 3 * q:3 * q + 3, 3 * l:3 * l + 3] = blk[:, :, l]
    return out


def _split(GB):
    """The blocks G0..G3 (B, N, 4, 3, 3) of g_Bd (B, N, 12, 12): rows 3q..3q+2, columns 3l..3l+2."""
    B, N = GB.shape[:2]
    G = GB.reshape(B, N, 4, 3, 4, 3).transpose(0, 1, 4, 2, 3, 5)    # (B, N, leg, q, 3, 3)
    return [G[:, :, :, q] for q in range(4)]


def forward(mass, inertia, r_feet, xref, dt):
    """The closed form -> Ad (B,12,12), Bd (B,N,12,12) in float64 (gd is a constant of dt)."""
    mass, inertia, r_feet, xref = map(f32, (mass, inertia, r_feet, xref))
    return _forward64(mass, inertia, r_feet, xref, float(np.float32(dt)))


def _forward64(mass, inertia, r_feet, xref, dt):
    B, N = r_feet.shape[:2]
    h2 = 0.5 * dt * dt
    minv, J, c, s, Rt = _robot(mass, inertia, xref)
    W = np.einsum("bij,bkljm->bklim", J, skew(r_feet))
    V = np.einsum("bij,bkljm->bklim", Rt, W)
    eye = np.broadcast_to(np.eye(3), (B, N, 4, 3, 3)) * minv[:, None, None, None, None]
    Bd = _blocks(B, N, h2 * eye, h2 * V, dt * eye, dt * W)
    Ad = np.tile(np.eye(12), (B, 1, 1))
    Ad[:, 0:3, 6:9] += dt * np.eye(3)
    Ad[:, 3:6, 9:12] += dt * Rt
    return Ad, Bd


def ref_vjp(mass, inertia, r_feet, xref, dt, g_Ad=None, g_Bd=None):
    """-> (vals, S): dicts over VJP_OUTPUTS; vals of the outputs' shapes, S (B,) each."""
    mass, inertia, r_feet, xref = map(f32, (mass, inertia, r_feet, xref))
    B, N = r_feet.shape[:2]
    dt = float(np.float32(dt))                            # the C-ABI's dt is a float
    h2 = 0.5 * dt * dt
    a = np.abs
    GA = np.zeros((B, 12, 12)) if g_Ad is None else np.asarray(g_Ad, np.float64)
    GB = np.zeros((B, N, 12, 12)) if g_Bd is None else np.asarray(g_Bd, np.float64)
    G0, G1, G2, G3 = _split(GB)
    minv, J, c, s, Rt = _robot(mass, inertia, xref)
    S = skew(r_feet)
    tr = lambda G: np.einsum("bklii->b", G)                                  # noqa: E731
    g_minv = h2 * tr(G0) + dt * tr(G2)
    M = dt * G3 + h2 * np.einsum("bji,bkljm->bklim", Rt, G1)                 # Rt' G1
    g_r = unskew(np.einsum("bji,bkljm->bklim", J, M))                        # J' M
    g_J = np.einsum("bklij,bklmj->bim", M, S)                                # sum M S'
    g_I = -np.einsum("bji,bjk,bmk->bim", J, g_J, J)                          # -J' g_J J'
    W = np.einsum("bij,bkljm->bklim", J, S)
    g_Rt = dt * GA[:, 3:6, 9:12] + h2 * np.einsum("bklij,bklmj->bim", G1, W)  # sum G1 W'
    g_yaw = -s * g_Rt[:, 0, 0] + c * g_Rt[:, 0, 1] - c * g_Rt[:, 1, 0] - s * g_Rt[:, 1, 1]
    vals = dict(mass=-g_minv / mass ** 2, inertia=g_I, r_feet=g_r, yaw=g_yaw)
    # the scales: the same formulas on absolute values
    aJ, aS, aRt = a(J), a(S), a(Rt)
    s_minv = h2 * tr(a(G0)) + dt * tr(a(G2))
    aM = dt * a(G3) + h2 * np.einsum("bji,bkljm->bklim", aRt, a(G1))
    agS = np.einsum("bji,bkljm->bklim", aJ, aM)
    s_r = np.stack([agS[..., 2, 1] + agS[..., 1, 2], agS[..., 0, 2] + agS[..., 2, 0],
                    agS[..., 1, 0] + agS[..., 0, 1]], axis=-1)
    s_I = np.einsum("bji,bjk,bmk->bim", aJ, np.einsum("bklij,bklmj->bim", aM, aS), aJ)
    aW = np.einsum("bij,bkljm->bklim", aJ, aS)
    s_Rt = dt * a(GA[:, 3:6, 9:12]) + h2 * np.einsum("bklij,bklmj->bim", a(G1), aW)
    s_yaw = (a(c) + a(s)) * s_Rt[:, :2, :2].sum(axis=(1, 2))
    scale = dict(mass=s_minv / mass ** 2, inertia=s_I.reshape(B, -1).max(axis=1),
                 r_feet=s_r.reshape(B, -1).max(axis=1), yaw=s_yaw)
    return vals, scale


def ref_jvp(mass, inertia, r_feet, xref, dt, d_mass=None, d_inertia=None, d_r_feet=None,
            d_xref=None):
    """-> (vals, S): dicts over JVP_OUTPUTS; vals float64 of the outputs' shapes, S (B,) each."""
    mass, inertia, r_feet, xref = map(f32, (mass, inertia, r_feet, xref))
    B, N = r_feet.shape[:2]
    dt = float(np.float32(dt))                            # the C-ABI's dt is a float
    h2 = 0.5 * dt * dt
    a = np.abs
    dm = np.zeros(B) if d_mass is None else f32(d_mass)
    dI = np.zeros((B, 3, 3)) if d_inertia is None else f32(d_inertia)
    dr = np.zeros((B, N, 4, 3)) if d_r_feet is None else f32(d_r_feet)
    dx5 = np.zeros((B, N)) if d_xref is None else f32(d_xref)[:, :, 5]
    minv, J, c, s, Rt = _robot(mass, inertia, xref)
    S, dS = skew(r_feet), skew(dr)
    dminv = -dm / mass ** 2
    dJ = -np.einsum("bij,bjk,bkm->bim", J, dI, J)
    dyaw = dx5.sum(axis=1) / N
    dRt = np.zeros((B, 3, 3))
    dRt[:, 0, 0], dRt[:, 0, 1], dRt[:, 1, 0], dRt[:, 1, 1] = -s * dyaw, c * dyaw, -c * dyaw, -s * dyaw
    mul = lambda A, X: np.einsum("bij,bkljm->bklim", A, X)                   # noqa: E731
    W = mul(J, S)
    dW = mul(dJ, S) + mul(J, dS)
    dV = mul(dRt, W) + mul(Rt, dW)
    eye = np.broadcast_to(np.eye(3), (B, N, 4, 3, 3))
    e = lambda v: eye * v[:, None, None, None, None]                         # noqa: E731
    d_Bd = _blocks(B, N, h2 * e(dminv), h2 * dV, dt * e(dminv), dt * dW)
    d_Ad = np.zeros((B, 12, 12))
    d_Ad[:, 3:6, 9:12] = dt * dRt
    # the scales
    aJ, aRt = a(J), a(Rt)
    adyaw = a(dx5).sum(axis=1) / N
    adRt = np.zeros((B, 3, 3))                            # |dyaw| [[|s|, |c|, 0], [|c|, |s|, 0], 0]
    adRt[:, 0, 0] = adRt[:, 1, 1] = a(s) * adyaw
    adRt[:, 0, 1] = adRt[:, 1, 0] = a(c) * adyaw
    adJ = np.einsum("bij,bjk,bkm->bim", aJ, a(dI), aJ)
    aW = mul(aJ, a(S))
    adW = mul(adJ, a(S)) + mul(aJ, a(dS))
    adV = mul(adRt, aW) + mul(aRt, adW)
    sB = _blocks(B, N, h2 * e(a(dminv)), h2 * adV, dt * e(a(dminv)), dt * adW)
    scale = dict(Ad=dt * adRt.reshape(B, -1).max(axis=1), Bd=sB.reshape(B, -1).max(axis=1))
    return dict(Ad=d_Ad, Bd=d_Bd), scale


def worst_ratio(got, vals, S, tol=TOL, rel=0.0):
    """name -> max over robots and entries of |got - ref| / (rel |ref| + tol S_robot) for the
    outputs present in got; where the bound is 0, 0 if got equals the reference, else inf."""
    out = {}
    for n, g in got.items():
        ref = np.asarray(vals[n], np.float64)
        g = np.asarray(g, np.float64).reshape(ref.shape)
        B = ref.shape[0]
        err = np.abs(g - ref).reshape(B, -1)
        bound = rel * np.abs(ref).reshape(B, -1) + tol * np.asarray(S[n])[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))
        out[n] = float(r.max()) if r.size else 0.0
    return out


def random_case(rng, B, N, base):
    """Inputs from ``base`` (a synth.make_config(3, ..) batch): its first B robots and N steps, as
    fp32; with random fp64 gradients ~ N(0, 1) and fp32 tangents scaled to each input."""
    c = dict(mass=np.float32(base["m"][:B]), inertia=np.float32(base["I_world"][:B]),
             r_feet=np.ascontiguousarray(np.float32(base["r_legs"][:B, :N])),
             xref=np.ascontiguousarray(np.float32(base["xref"][:B, :N])), dt=float(base["dt"]))
    c["g_Ad"] = rng.standard_normal((B, 12, 12))
    c["g_Bd"] = rng.standard_normal((B, N, 12, 12))
    c["d_mass"] = np.float32(rng.standard_normal(B))
    c["d_inertia"] = np.float32(0.01 * rng.standard_normal((B, 3, 3)))
    c["d_r_feet"] = np.float32(0.1 * rng.standard_normal((B, N, 4, 3)))
    c["d_xref"] = np.float32(rng.standard_normal((B, N, 12)))
    return c


def inputs(c):
    return [c[k] for k in ("mass", "inertia", "r_feet", "xref")] + [c["dt"]]
