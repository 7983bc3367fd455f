"""The one-wave-per-SIMD solve kernels (NC 144 / 160 / 192) at the edges of their register
classes, forced at a small batch with Plan.set_team(0): the NC 144 / 160 kernel runs the
gradient's predicated form, and every one of them the plain sweep and the first-touch staging
(contact bytes and whole Bd rows in the first round of loads, stance columns scattered by ballot).

Free-force counts n (3 per stance (step, leg) pair): 129 is the smallest NC 144 instance (33
pivot groups: the last 4-pivot step holds one real pivot and three padding pivots), 144 fills
NC 144, 147 and 159 are the edges of NC 160, 162 and 192 those of NC 192, and 0 is an all-swing
instance.  Each mask is a config-2 instance's own contact table with its latest stance entries
turned to swing, or its earliest swing entries to stance, until the count fits (192: every
foot in stance at every step).  The certified optima are tests/golden/qp_heavy_edges.npz
(tests/golden/make_heavy_edges.py: oracle/tight_solver.py, KKT residuals below 1e-8, with the
digest of the inputs they belong to).

Tolerance (BASELINE.json north_star, as tests/test_gpu_parity.py): contact forces within 1e-4
relative of the KKT-certified float64 optimum, status 1 (parity_util.assert_verified: a small
batch may hold at most one status 2, which keeps test_gpu_terrain's 1e-3 bar).
"""
import numpy as np
import pytest

from parity_util import (load_fixture, rel_err_U, split_w, rollout64, assert_verified,
                         input_digest)

pytestmark = pytest.mark.gpu
TOL_U = 1e-4
KEYS = ("Ad", "Bd", "gd", "x0", "xref", "contact")
EDGE_N = (129, 144, 147, 159, 162, 192, 0)
PER_N = 5
SHORT = dict(N=8, per_n=3, targets=(96, 93, 48, 0), seed=29)


def _count(contact):
    return (contact != 0).reshape(contact.shape[0], -1).sum(1)


def edge_batch(N=16, per_n=PER_N, targets=EDGE_N, seed=23):
    """per_n instances for each free-force count in `targets`, in that order."""
    from cmpc import synth
    pool = synth.make_batch(512, seed=seed, mixed=True, N=N)
    cnt = _count(pool["contact"])
    out = {k: [] for k in KEYS}
    used = set()
    for n in targets:
        want = n // 3
        # the instances whose own stance count is nearest
        cand = [i for i in np.argsort(np.abs(cnt - want), kind="stable") if i not in used]
        for i in cand[:per_n]:
            used.add(int(i))
            ct = pool["contact"][i].copy()           # (4, N)
            have = int(cnt[i])
            if have > want:    # latest stance entries to swing
                for k, l in [(k, l) for k in range(N - 1, -1, -1) for l in range(4) if ct[l, k]][:have - want]:
                    ct[l, k] = 0
            elif have < want:  # earliest swing entries to stance (their Bd columns have a zero lever)
                for k, l in [(k, l) for k in range(N) for l in range(4) if not ct[l, k]][:want - have]:
                    ct[l, k] = 1
            assert int((ct != 0).sum()) == want
            for key in KEYS:
                out[key].append(ct if key == "contact" else pool[key][i])
    return {k: np.stack(v) for k, v in out.items()}


def _one_wave_plan(N=16, max_batch=64):
    from cmpc import Plan, SolverParams
    p = Plan(SolverParams(N=N, max_batch=max_batch))
    p.set_team(0)
    return p


@pytest.fixture(scope="module")
def edges():
    """The edge batch and its certified optima."""
    fx = load_fixture("qp_heavy_edges.npz")
    b = edge_batch()
    assert input_digest(b, np.arange(len(b["Ad"]))) == str(fx["digest"]), "generator drifted"
    ref = fx["w"]
    ref.setflags(write=False)
    return b, ref


def _check(w, st, ref, N=16):
    ok = assert_verified(st)
    err = rel_err_U(w, ref, N=N)
    print("status", st.tolist())
    print("rel err", err.tolist())
    for i in range(len(err)):
        assert err[i] <= (TOL_U if ok[i] else 1e-3), (i, int(st[i]), err[i])


def test_edge_counts_parity(edges):
    from cmpc import solve_batch
    b, ref = edges
    assert (3 * _count(b["contact"])).tolist() == [n for n in EDGE_N for _ in range(PER_N)]
    p = _one_wave_plan()
    names = p.solve_kernels(len(ref))
    assert all("group" in k for k in names if k), names
    w, st, it = solve_batch(b, plan=p)
    _check(w, st, ref)
    Xg, Ug = split_w(w.astype(np.float64))
    swing = 3 * _count(b["contact"]) == 0
    assert np.all(Ug[swing] == 0)
    assert np.max(np.abs(Xg - rollout64(b, Ug))) < 1e-4


def test_reversed_order_bitwise(edges):
    """The same batch in reversed instance order: every instance lands on another wave, after
    other instances and another queue pop; its outputs are bitwise the same."""
    from cmpc import solve_batch
    b, _ = edges
    p = _one_wave_plan()
    w0, s0, i0 = solve_batch(b, plan=p)
    w1, s1, i1 = solve_batch({k: b[k][::-1].copy() for k in KEYS}, plan=p)
    w1, s1, i1 = w1[::-1], s1[::-1], i1[::-1]
    same = np.all(w0.view(np.uint32) == w1.view(np.uint32), axis=1) & (s0 == s1) & (i0 == i1)
    assert same.all(), np.flatnonzero(~same).tolist()


def test_general_step_matrix_edges(edges):
    """A step matrix that is not I + N, N^2 = 0 (the attitude-damped Ad of
    test_general_step_matrix_heavy_bins): the gradient's squared-power scans behind the
    predicated form, on the smallest NC 144 instance (n = 129) and the largest NC 160 one
    (n = 159).  Certified on the CPU as there (oracle/active_set.py, seeded by the GPU's answer);
    a general A keeps the relative multiplier test, so a loose acceptance is status 2: the rule
    of test_general_step_matrix_one_wave_latency (at most one status 2, within 1e-3)."""
    from cmpc import solve_batch
    from oracle import active_set, mpc_qp
    b0, _ = edges
    pick = [EDGE_N.index(n) * PER_N for n in (129, 159)]
    b = {k: b0[k][pick].astype(np.float64) for k in KEYS}
    for r in range(3, 6):
        b["Ad"][:, r, r] = 0.999
    Nm = b["Ad"][0].astype(np.float32) - np.eye(12, dtype=np.float32)
    assert np.any(Nm @ Nm != 0)
    w, st, it = solve_batch(b, plan=_one_wave_plan())
    print("status", st.tolist(), "iters", it.tolist())
    ok = assert_verified(st)
    for i in range(len(pick)):
        qp = mpc_qp.build_qp(b["Ad"][i], b["Bd"][i], b["gd"][i], b["x0"][i], b["xref"][i].T,
                             b["contact"][i])
        r = active_set.certified_optimum(qp, w[i].astype(np.float64))
        assert max(r["kkt"].values()) <= active_set.CERT_TOL, i
        err = rel_err_U(w[i:i + 1], r["w"][None])[0]
        print(i, "rel err", err)
        assert err <= (TOL_U if ok[i] else 1e-3), (i, int(st[i]), err)


def test_short_horizon():
    """N = 8: the gradient's lanes c >= N hold no step.  At this horizon every instance has at
    most 96 free forces (the NC 96 bin, two waves per SIMD), so the predicated form is the team
    kernel's: the batch is solved with team mode forced (predicated: lanes c >= N read step 0
    and are zeroed) and with team mode off (rolled: those lanes skip the loop).  Counts 96 (every
    foot in stance), 93, 48 and 0."""
    from cmpc import solve_batch
    fx = load_fixture("qp_heavy_edges.npz")
    b = edge_batch(**SHORT)
    assert input_digest(b, np.arange(len(b["Ad"]))) == str(fx["digest8"]), "generator drifted"
    ref = fx["w8"]
    p = _one_wave_plan(N=8)
    for team in (1 << 40, 0):
        p.set_team(team)
        w, st, it = solve_batch(b, plan=p)
        assert w.shape == (len(ref), 24 * 8)
        _check(w, st, ref, N=8)
