"""GPU: one closed-loop tick of ``ClosedLoop`` (cmpc/closed_loop.py) against the oracle chain,
teacher-forced: a free-running comparison of a feedback loop diverges chaotically, so at every
tick the device's own state is the oracle's input and one tick is checked.

Before a tick x, feet, contact, t, pos_des, w and y are copied; after it every buffer the tick
left behind is compared with what the oracles make of that snapshot:

  lever, I_world      feet - p to one float32 rounding; R I_b R' within the bound derived below
  xref, ct, rf        oracle/traj_ref.py fed the snapshot and the device's lever (contact table
                      and pos_des exact; xref and levers to test_gpu_traj.py's bar)
  Ad, Bd, gd          synth.discretize fed the device's I_world, rf, xref (test_gpu_dynamics.py's
                      bar)
  w_init, y_init      the previous w (its U part) and y shifted one step, last step repeated:
                      bitwise
  w, status           6 robots per tick (rotating through the batch) and every status-2 robot:
                      the KKT-certified optimum (<= 1e-8) of the QP assembled from the device's
                      own float32 data; 1e-4 relative on U at status 1, 1e-3 at status 2
  x, feet, contact    oracle/srb_ref.py stepping the snapshot under w[:, 192:204] from the
                      snapshot's time with h = dt / 20: test_gpu_srb.py's tolerances.  A plant
                      that read another row than u_0, the forces of before the solve or another
                      time fails here.
  t                   snapshot + dt, exactly

Bound on I_world.  eps = 2^-24.  A float32 sin / cos is within 4 ulp <= 8 eps of the true value
(the OpenCL full-profile bound, which the device's math library meets).  An entry of R is a sum
of at most two products of at most three such values: relative to the magnitudes of its terms it
carries 3 * 8 eps (values) + 2 eps (multiplications) + eps (the addition) = 27 eps.  The torch
expression forms RI = sum_j R_ij I_jk (one multiplication, two additions in some order: 3 eps;
I_b is float32 data, exact) and I_w = sum_k RI_ik R_lk (a second entry of R, 27 eps, and 3 eps
again).  Each of the 9 triple products R_ij I_jk R_lk of an entry is therefore off by at most
(27 + 3 + 27 + 3) eps = 60 eps to first order, (1 + eps)^60 - 1 < 61 eps in all, and
|I_w - R I_b R'| <= k eps (Rm |I_b| Rm')  with k = 64,
Rm the matrix of summed term magnitudes of R (|cy sp sr| + |sy cr| and so on; Rm >= |R|).
R and R' exchanged in this product change entries of I_w by 1e-2 of their size (rolled and
pitched robots with different principal inertias), four orders of magnitude above the bound.

Measured on an MI355X over the four cases: plant error / float32 yardstick at most p 1.00,
rpy 1.00, v 1.43, w 1.14, feet 1.44 (bar 8); 72 certified solves per case, all status 1, worst
relative error on U 1.3e-6.
"""
import numpy as np
import pytest

from srb_util import check_against_oracle, GROUPS
from test_gpu_closed_loop import _command
from test_gpu_dynamics import _close as _close_dyn
from test_gpu_traj import _close as _close_traj

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
K_INERTIA = 64
TICKS, EAGER = 12, 2


def _np(t):
    return t.detach().cpu().numpy().copy()


def _rot_terms(rpy):
    """float64 R = Rz Ry Rx of (B,3) angles and the matrix of summed term magnitudes."""
    r, p, y = rpy[:, 0], rpy[:, 1], rpy[:, 2]
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    z = np.zeros_like(r)
    a = np.array([[cy * cp, cy * sp * sr, cy * sp * cr], [sy * cp, sy * sp * sr, sy * sp * cr],
                  [-sp, cp * sr, cp * cr]])
    b = np.array([[z, -sy * cr, sy * sr], [z, cy * cr, -cy * sr], [z, z, z]])
    R = np.moveaxis(a + b, -1, 0)
    Rm = np.moveaxis(np.abs(a) + np.abs(b), -1, 0)
    return R, Rm


def _shift(a, B, N):
    a = a.reshape(B, N, 12)
    return np.concatenate([a[:, 1:], a[:, -1:]], 1).reshape(B, 12 * N)


@pytest.mark.parametrize("per_robot", [False, True], ids=["plan_constants", "per_robot"])
@pytest.mark.parametrize("size", ["team", "group"])
def test_tick_against_oracle_chain(plan, size, per_robot):
    import torch
    from cmpc import synth
    from cmpc.closed_loop import ClosedLoop
    from oracle import active_set, mpc_qp, traj_ref
    if size == "team":
        B = 48
        assert B <= plan.team_batch()
    else:
        B = plan.team_batch() + 40
        assert all(plan.solve_kernels(B))
    N = plan.params.N
    P = plan.params
    mu = np.full(B, P.mu)
    fz = np.full(B, P.fz_min)
    Q = np.tile(np.asarray(P.Q, np.float64), (B, 1))
    R = np.tile(np.asarray(P.R, np.float64), (B, 1))
    kw = {}
    if per_robot:
        tr, wt = synth.make_terrain(B, seed=12), synth.make_weights(B, seed=13)
        mu, fz, Q, R = tr["mu"], tr["fz_min"], wt["Q"], wt["R"]
        kw = dict(mu=mu, fz_min=fz, Q=Q, R=R)
    cl = ClosedLoop(B, plan=plan, seed=5, **kw)
    cl.set_command(_command(B, np.random.default_rng(6)))
    cmd = _np(cl.cmd).astype(np.float64)
    gait, hip = _np(cl.gait), _np(cl.hip).astype(np.float64)
    mass, Ib = _np(cl.mass).astype(np.float64), _np(cl.I_body).astype(np.float64)
    h = cl.dt / cl.nsub
    landed = lifted = 0
    worst = dict(st1=0.0, st2=0.0, **{g: 0.0 for g in GROUPS})
    n_cert = 0
    for k in range(TICKS):
        if k == EAGER:
            cl.capture()
        torch.cuda.synchronize(cl.dev)
        s = {n: _np(getattr(cl, n)) for n in ("x", "feet", "contact", "t", "pos_des", "w", "y")}
        cl.tick()
        torch.cuda.synchronize(cl.dev)
        a = {n: _np(getattr(cl, n)) for n in (
            "x", "feet", "contact", "t", "pos_des", "w", "y", "lever", "I_world", "xref", "ct",
            "rf", "Ad", "Bd", "gd", "w_init", "y_init", "status")}
        x0 = s["x"].astype(np.float64)

        # --- inputs to the QP
        lever = s["feet"].astype(np.float64) - x0[:, None, 0:3]
        assert np.all(np.abs(a["lever"] - lever) <= EPS32 * np.abs(lever)), k
        Rr, Rm = _rot_terms(x0[:, 3:6])
        Iw = Rr @ Ib @ np.swapaxes(Rr, 1, 2)
        bound = K_INERTIA * EPS32 * (Rm @ np.abs(Ib) @ np.swapaxes(Rm, 1, 2))
        assert np.all(np.abs(a["I_world"] - Iw) <= bound), (k, np.abs(a["I_world"] - Iw).max())
        dev_lever = a["lever"].astype(np.float64)
        pd_o, xref_o, ct_o, rf_o = traj_ref.generate_traj(x0, s["pos_des"], cmd, s["t"], gait,
                                                          dev_lever, hip, cl.dt, N)
        np.testing.assert_array_equal(a["ct"], ct_o)
        np.testing.assert_array_equal(a["pos_des"], pd_o)
        assert _close_traj(a["xref"], xref_o), k
        assert _close_traj(a["rf"], rf_o), k
        xref64 = a["xref"].astype(np.float64)
        Ad_o, Bd_o, gd_o = synth.discretize(mass, a["I_world"].astype(np.float64),
                                            a["rf"].astype(np.float64), xref64[:, :, 5].mean(1),
                                            cl.dt)
        assert _close_dyn(a["Ad"], Ad_o) and _close_dyn(a["Bd"], Bd_o), k
        assert _close_dyn(a["gd"], gd_o), k

        # --- warm start
        if k >= 1:
            assert np.array_equal(a["w_init"][:, 12 * N:], _shift(s["w"][:, 12 * N:], B, N)), k
            assert np.array_equal(a["y_init"], _shift(s["y"], B, N)), k

        # --- solve
        st = a["status"]
        assert np.all((st == 1) | (st == 2)), (k, np.unique(st, return_counts=True))
        assert np.sum(st == 2) <= 1, (k, np.flatnonzero(st == 2))
        for i in sorted(set((6 * k + np.arange(6)) % B) | set(np.flatnonzero(st == 2))):
            qp = mpc_qp.build_qp(a["Ad"][i].astype(np.float64), a["Bd"][i].astype(np.float64),
                                 a["gd"][i].astype(np.float64), x0[i], xref64[i].T, a["ct"][i],
                                 Q=Q[i], R=R[i], mu=float(mu[i]), fz_min=float(fz[i]))
            w_i = a["w"][i].astype(np.float64)
            r = active_set.certified_optimum(qp, w_i)
            assert max(r["kkt"].values()) <= 1e-8, (k, i, r["kkt"])
            Ur = r["w"][12 * N:]
            err = float(np.max(np.abs(w_i[12 * N:] - Ur)) / np.max(np.abs(Ur)))
            key = "st1" if st[i] == 1 else "st2"
            worst[key] = max(worst[key], err)
            assert err <= (1e-4 if st[i] == 1 else 1e-3), (k, i, int(st[i]), err)
            n_cert += 1

        # --- hand-off to the plant, and the time
        inp = dict(x=x0, feet=s["feet"].astype(np.float64), contact_state=s["contact"],
                   t_now=s["t"], gait=gait, mass=mass, inertia_body=Ib,
                   force=a["w"][:, 12 * N:12 * N + 12].astype(np.float64), hip=hip)
        ratio = check_against_oracle((a["x"], a["feet"], a["contact"]), inp, h, cl.nsub,
                                     label=f"tick {k}:")
        for g in GROUPS:
            worst[g] = max(worst[g], ratio[g])
        assert np.array_equal(a["t"], s["t"] + cl.dt), k
        if k >= EAGER:                                   # under the captured graph
            landed += int(np.sum(a["contact"] & ~s["contact"] != 0))
            lifted += int(np.sum(s["contact"] & ~a["contact"] != 0))
    print(f"B={B} per_robot={per_robot}: {n_cert} certified solves, worst", worst,
          "robots landing", landed, "lifting", lifted)
    assert landed > 0 and lifted > 0
