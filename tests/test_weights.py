"""CPU: the host side of per-instance cost weights -- the Q / R fields appended to cmpc_solve_io
and its entry's size rule, synth.make_weights, the sharding of the optional (B, 12) stacks, and
the certificates of tests/golden/qp_weights.npz."""
import ctypes
import os
import shutil
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO
from parity_util import load_fixture, input_digest


@pytest.fixture(scope="module")
def lib():
    from cmpc import _lib
    from cmpc.build import build_library, LIB
    if not LIB.exists():
        build_library()
    return _lib.load()


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of cmpc_solve_io as a C compiler lays out include/cmpc.h, Q and R (its
    last two fields) included."""
    from cmpc import _lib
    from cmpc.build import hipcc
    names = [n for n, _ in _lib.CSolveIO._fields_]
    assert names[-2:] == ["Q", "R"] and names[-3] == "iters"
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cmpc.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(cmpc_solve_io));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(cmpc_solve_io, {n}));\n' for n in names) +
                   '  printf("%d\\n", CMPC_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    cc = shutil.which("cc") or shutil.which("gcc")
    cmd = [cc, str(src)] if cc else [hipcc(), "-x", "c", str(src)]
    subprocess.run(cmd + [f"-I{REPO / 'include'}", "-o", str(exe)], check=True, timeout=120)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True,
                                           timeout=60).stdout.split()]
    assert vals[0] == ctypes.sizeof(_lib.CSolveIO)
    assert vals[1:-1] == [getattr(_lib.CSolveIO, n).offset for n in names]
    assert vals[-1] == 6                        # the struct grew at its end: no ABI bump


def test_a_struct_that_stops_before_Q_is_accepted(lib):
    """A caller compiled against the header before Q / R passes that header's sizeof: the
    argument checks accept it (it reaches the null-plan test, the last one before the plan is
    read), as they accept the full struct and one with Q / R set."""
    from cmpc import _lib
    old = _lib.CSolveIO.Q.offset
    assert old == ctypes.sizeof(_lib.CSolveIO) - 2 * ctypes.sizeof(ctypes.c_void_p)
    for size, ptrs in ((old, {}), (ctypes.sizeof(_lib.CSolveIO), {}),
                       (ctypes.sizeof(_lib.CSolveIO), dict(Q=64, R=64)),
                       # garbage where Q / R would be, past the caller's size: never read
                       (old, dict(Q=64, R=64, y_out=64))):
        io = _lib.CSolveIO()
        io.size = size
        for k, v in ptrs.items():
            setattr(io, k, v)
        assert lib.cmpc_solve_io_run(None, 1, ctypes.byref(io), None) == -22
        msg = _lib.last_error(lib)
        assert "cmpc_solve_io_run" in msg and "null plan" in msg, msg
    short = _lib.CSolveIO()
    short.size = 4
    assert lib.cmpc_solve_io_run(None, 1, ctypes.byref(short), None) == -22
    assert "size" in _lib.last_error(lib)


def _recipe(seed, span, lo, hi):
    """The recipe of make_golden_weights.py's header, written out: Q first, then R, from one
    generator."""
    rng = np.random.default_rng(seed)
    q0 = np.array([1, 1, 50, 10, 20, 1, 2, 2, 1, 1, 1, 1], np.float64)
    Q = q0 * np.exp(rng.uniform(-np.log(span), np.log(span), (34, 12)))
    R = np.exp(rng.uniform(np.log(lo), np.log(hi), (34, 12)))
    return Q, R


def test_make_weights():
    from cmpc import synth, SolverParams
    assert tuple(synth.Q_DEFAULT) == tuple(SolverParams().Q)
    before = input_digest(synth.make_config(2, B=64), np.arange(64))
    a, b = synth.make_weights(1000, seed=5), synth.make_weights(1000, seed=5)
    assert all(np.array_equal(a[k], b[k]) for k in ("Q", "R")) and set(a) == {"Q", "R"}
    c = synth.make_weights(1000, seed=6)
    assert not np.array_equal(a["Q"], c["Q"]) and not np.array_equal(a["R"], c["R"])
    q0 = np.asarray(synth.Q_DEFAULT, np.float64)
    for v in (a["Q"], a["R"]):
        assert v.shape == (1000, 12) and v.dtype == np.float64
        assert np.array_equal(v, v.astype(np.float32).astype(np.float64))
    assert np.all(a["Q"] >= q0 / 4) and np.all(a["Q"] <= q0 * 4)
    assert np.all(a["R"] >= 2.5e-6) and np.all(a["R"] <= 1e-4)
    # log-uniform: the spread in the logarithm is that of U(-ln 4, ln 4), sigma = 2 ln 4 / sqrt(12)
    assert abs(np.log(a["Q"] / q0).std() - 2 * np.log(4) / np.sqrt(12)) < 0.02
    assert abs(np.log(a["R"]).std() - np.log(1e-4 / 2.5e-6) / np.sqrt(12)) < 0.03
    wide = synth.make_weights(64, seed=22, q_span=10.0, r=(1e-6, 1e-3))
    assert np.all(wide["Q"] >= q0 / 10) and np.all(wide["Q"] <= q0 * 10)
    assert wide["R"].min() >= 1e-6 and wide["R"].max() <= 1e-3 and wide["R"].max() > 1e-4
    # its generator is its own: the batch generators draw what they drew
    assert input_digest(synth.make_config(2, B=64), np.arange(64)) == before


def test_fixture_draws():
    """The fixture's weights are make_weights' and the recipe's: set A default_rng(21), span 4,
    R in [2.5e-6, 1e-4]; set B default_rng(22), span 10, R in [1e-6, 1e-3], then the zeroed Q
    entries.  Its inputs are qp_terrain.npz's."""
    from cmpc import synth
    fx, ft = load_fixture("qp_weights.npz"), load_fixture("qp_terrain.npz")
    for k in ("Ad", "Bd", "gd", "x0", "xref", "contact"):
        assert np.array_equal(fx[k], ft[k])
    A = synth.make_weights(34, seed=21)
    assert np.array_equal(fx["Q_A"], A["Q"].astype(np.float32))
    assert np.array_equal(fx["R_A"], A["R"].astype(np.float32))
    QA, RA = _recipe(21, 4.0, 2.5e-6, 1e-4)
    assert np.allclose(fx["Q_A"], QA, rtol=1e-6, atol=0) and np.allclose(fx["R_A"], RA, rtol=1e-6, atol=0)
    B = synth.make_weights(34, seed=22, q_span=10.0, r=(1e-6, 1e-3))
    QB, RB = _recipe(22, 10.0, 1e-6, 1e-3)
    for Q in (B["Q"], QB):
        Q[::5, 0] = 0.0
        Q[1::5, 5] = 0.0
    assert np.array_equal(fx["Q_B"], B["Q"].astype(np.float32))
    assert np.array_equal(fx["R_B"], B["R"].astype(np.float32))
    assert np.allclose(fx["Q_B"], QB, rtol=1e-6, atol=0) and np.allclose(fx["R_B"], RB, rtol=1e-6, atol=0)
    assert np.sum(fx["Q_B"] == 0) == 14 and np.all(fx["Q_A"] > 0)
    assert np.all(fx["R_A"] > 0) and np.all(fx["R_B"] > 0)


def test_fixture_certificates():
    """The stored optima are KKT points of the QPs with the stored per-instance weights (no
    solve), for every instance of both sets."""
    from oracle import mpc_qp
    fx = load_fixture("qp_weights.npz")
    assert fx["w_A"].shape == (34, 384) and fx["kkt_A"].max() <= 1e-8 and fx["kkt_B"].max() <= 1e-8
    nf = 3 * (fx["contact"] != 0).reshape(34, -1).sum(1)
    assert np.any(nf <= 128) and np.any((nf > 128) & (nf <= 160)) and np.sum(nf > 160) >= 2
    for tag in ("A", "B"):
        for i in range(34):
            f64 = {k: np.asarray(fx[k][i], np.float64) for k in ("Ad", "Bd", "gd", "x0", "xref")}
            qp = mpc_qp.build_qp(f64["Ad"], f64["Bd"], f64["gd"], f64["x0"], f64["xref"].T,
                                 fx["contact"][i], Q=fx[f"Q_{tag}"][i].astype(np.float64),
                                 R=fx[f"R_{tag}"][i].astype(np.float64), mu=0.8, fz_min=10.0)
            k = mpc_qp.kkt_residuals(qp, fx[f"w_{tag}"][i], fx[f"lam_x_{tag}"][i], fx[f"lam_a_{tag}"][i])
            assert max(k.values()) <= 1e-8, (i, tag, k)
    # the weights matter: the two sets' optima differ
    assert np.max(np.abs(fx["w_A"][:, 192:] - fx["w_B"][:, 192:])) > 1.0


def test_shard_batch_slices_optional_stacks():
    from cmpc import dist as cdist, synth
    full = synth.make_config(2, B=7)
    assert set(cdist.shard_batch(full, 1, 2)) == set(cdist.FIELDS)
    assert cdist.FIELDS == ("Ad", "Bd", "gd", "x0", "xref", "contact")
    assert cdist.TERRAIN == ("mu", "fz_min") and cdist.WEIGHTS == ("Q", "R")
    full.update(synth.make_weights(7, seed=1))
    for r in range(2):
        lo, hi = cdist.shard_bounds(7, r, 2)
        s = cdist.shard_batch(full, r, 2)
        assert set(s) == set(cdist.FIELDS) | {"Q", "R"}
        assert s["Q"].shape == (hi - lo, 12)
        assert np.array_equal(s["Q"], full["Q"][lo:hi]) and np.array_equal(s["R"], full["R"][lo:hi])
    full.update(synth.make_terrain(7, seed=1))
    assert set(cdist.shard_batch(full, 0, 2)) == set(cdist.FIELDS) | {"Q", "R", "mu", "fz_min"}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, B, N, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cmpc import dist as cdist, synth
        full = synth.make_config(2, B=B)
        full.update(synth.make_weights(B, seed=3))
        full.update(synth.make_terrain(B, seed=3))
        keys = cdist.FIELDS + cdist.WEIGHTS
        batch = None
        if rank == 0:
            batch = {k: torch.as_tensor(full[k], dtype=torch.uint8 if k == "contact" else torch.float32)
                     for k in keys + cdist.TERRAIN}
        mine = cdist.scatter_batch(batch, B, N, "cpu", weights=True)
        lo, hi = cdist.shard_bounds(B, rank, world)
        ok = set(mine) == set(keys)
        ok = ok and all(np.array_equal(mine[k].numpy(), full[k][lo:hi].astype(mine[k].numpy().dtype))
                        for k in keys)
        ok = ok and mine["Q"].shape == (hi - lo, 12) and mine["R"].dtype == torch.float32
        both = cdist.scatter_batch(batch, B, N, "cpu", terrain=True, weights=True)
        ok = ok and set(both) == set(keys + cdist.TERRAIN)
        ok = ok and np.array_equal(both["R"].numpy(), full["R"][lo:hi].astype(np.float32))
        plain = cdist.scatter_batch(batch, B, N, "cpu")
        ok = ok and set(plain) == set(cdist.FIELDS)
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def test_scatter_weights_gloo_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, 5, 16, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == {0: True, 1: True}
