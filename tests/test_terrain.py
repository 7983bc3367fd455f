"""CPU: the host side of per-instance terrain -- the cmpc_solve_io struct and its entry's
argument checks, synth.make_terrain, the sharding of the optional stacks, and the certificates
of tests/golden/qp_terrain.npz."""
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


def _io(**ptrs):
    from cmpc import _lib
    io = _lib.CSolveIO()
    io.size = ctypes.sizeof(_lib.CSolveIO)
    for k, v in ptrs.items():
        setattr(io, k, v)
    return io


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of cmpc_solve_io as a C compiler lays out include/cmpc.h."""
    from cmpc import _lib
    from cmpc.build import hipcc
    names = [n for n, _ in _lib.CSolveIO._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cmpc.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(cmpc_solve_io));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(cmpc_solve_io, {n}));\n' for n in names) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    cc = shutil.which("cc") or shutil.which("gcc")
    cmd = [cc, str(src)] if cc else [hipcc(), "-x", "c", str(src)]
    subprocess.run(cmd + [f"-I{REPO / 'include'}", "-o", str(exe)], check=True, timeout=120)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True,
                                           timeout=60).stdout.split()]
    assert vals[0] == ctypes.sizeof(_lib.CSolveIO)
    assert vals[1:] == [getattr(_lib.CSolveIO, n).offset for n in names]


def test_entry_is_declared_and_exported(lib):
    from cmpc import _lib
    assert "cmpc_solve_io_run" in _lib.EXPORTS and hasattr(lib, "cmpc_solve_io_run")


def test_null_and_exclusive_arguments(lib):
    from cmpc import _lib
    assert lib.cmpc_solve_io_run(None, 1, None, None) == -22
    assert "cmpc_solve_io_run" in _lib.last_error(lib)
    assert lib.cmpc_solve_io_run(None, 1, ctypes.byref(_io()), None) == -22
    msg = _lib.last_error(lib)
    assert "cmpc_solve_io_run" in msg and "null plan" in msg
    # this solver's dual and the reference's multipliers together (never dereferenced: the
    # struct is refused before the plan or any array is touched)
    for pair in (dict(y_out=64, lam_out=64), dict(y_init=64, lam_init=64), dict(y_init=64, lam_out=64)):
        assert lib.cmpc_solve_io_run(None, 1, ctypes.byref(_io(**pair)), None) == -22
        msg = _lib.last_error(lib)
        assert "cmpc_solve_io_run" in msg and "exclusive" in msg
    short = _io()
    short.size = 4
    assert lib.cmpc_solve_io_run(None, 1, ctypes.byref(short), None) == -22
    assert "size" in _lib.last_error(lib)


def test_make_terrain():
    from cmpc import synth
    before = input_digest(synth.make_config(2, B=64), np.arange(64))
    a, b = synth.make_terrain(1000, seed=5), synth.make_terrain(1000, seed=5)
    assert all(np.array_equal(a[k], b[k]) for k in ("mu", "fz_min")) and set(a) == {"mu", "fz_min"}
    c = synth.make_terrain(1000, seed=6)
    assert not np.array_equal(a["mu"], c["mu"])
    for k, (lo, hi) in (("mu", (0.2, 1.0)), ("fz_min", (0.0, 20.0))):
        v = a[k]
        assert v.shape == (1000,) and v.dtype == np.float64
        assert np.array_equal(v, v.astype(np.float32).astype(np.float64))
        assert v.min() >= lo and v.max() <= hi and v.std() > 0.2 * (hi - lo)
    ice = synth.make_terrain(64, seed=6, mu=(0.2, 0.5))
    assert ice["mu"].min() >= 0.2 and ice["mu"].max() <= 0.5
    # its generator is its own: the batch generators draw what they drew
    assert input_digest(synth.make_config(2, B=64), np.arange(64)) == before
    fx = load_fixture("qp_terrain.npz")
    assert np.array_equal(fx["mu_A"], synth.make_terrain(34, seed=5)["mu"].astype(np.float32))
    assert np.array_equal(fx["fz_min_B"],
                          synth.make_terrain(34, seed=6, mu=(0.2, 0.5))["fz_min"].astype(np.float32))


def test_make_batch_draws_are_unchanged():
    """The fixture's first 32 instances are synth.make_batch(32, seed=77, mixed=True) in fp32."""
    from cmpc import synth
    fx = load_fixture("qp_terrain.npz")
    b = synth.make_batch(32, seed=77, mixed=True)
    assert input_digest(b, np.arange(32)) == input_digest(fx, np.arange(32))


def test_shard_batch_slices_optional_stacks():
    from cmpc import dist as cdist, synth
    full = synth.make_config(2, B=7)
    assert set(cdist.shard_batch(full, 1, 2)) == set(cdist.FIELDS)
    assert cdist.FIELDS == ("Ad", "Bd", "gd", "x0", "xref", "contact")
    full.update(synth.make_terrain(7, seed=1))
    for r in range(2):
        lo, hi = cdist.shard_bounds(7, r, 2)
        s = cdist.shard_batch(full, r, 2)
        assert set(s) == set(cdist.FIELDS) | {"mu", "fz_min"}
        assert np.array_equal(s["mu"], full["mu"][lo:hi]) and np.array_equal(s["fz_min"], full["fz_min"][lo:hi])


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
        full.update(synth.make_terrain(B, seed=3))
        batch = None
        if rank == 0:
            batch = {k: torch.as_tensor(full[k], dtype=torch.uint8 if k == "contact" else torch.float32)
                     for k in cdist.FIELDS + cdist.TERRAIN}
        mine = cdist.scatter_batch(batch, B, N, "cpu", terrain=True)
        lo, hi = cdist.shard_bounds(B, rank, world)
        ok = set(mine) == set(cdist.FIELDS + cdist.TERRAIN)
        ok = ok and all(np.array_equal(mine[k].numpy(), full[k][lo:hi].astype(mine[k].numpy().dtype))
                        for k in cdist.FIELDS + cdist.TERRAIN)
        ok = ok and mine["mu"].shape == (hi - lo,) and mine["mu"].dtype == torch.float32
        plain = cdist.scatter_batch(batch, B, N, "cpu")
        ok = ok and set(plain) == set(cdist.FIELDS)
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def test_scatter_terrain_gloo_world2():
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


def test_fixture_certificates():
    """The stored optima are KKT points of the QPs with the stored per-instance terrain (no
    solve), and of every solve-kernel class."""
    from oracle import mpc_qp
    fx = load_fixture("qp_terrain.npz")
    assert fx["w_A"].shape == (34, 384) and fx["kkt_A"].max() <= 1e-8 and fx["kkt_B"].max() <= 1e-8
    nf = 3 * (fx["contact"] != 0).reshape(34, -1).sum(1)
    assert np.any(nf <= 128) and np.any((nf > 128) & (nf <= 160)) and np.sum(nf > 160) >= 2
    for i, tag in ((0, "A"), (13, "B"), (32, "A"), (33, "B")):
        f64 = {k: np.asarray(fx[k][i], np.float64) for k in ("Ad", "Bd", "gd", "x0", "xref")}
        qp = mpc_qp.build_qp(f64["Ad"], f64["Bd"], f64["gd"], f64["x0"], f64["xref"].T,
                             fx["contact"][i], mu=float(fx[f"mu_{tag}"][i]),
                             fz_min=float(fx[f"fz_min_{tag}"][i]))
        k = mpc_qp.kkt_residuals(qp, fx[f"w_{tag}"][i], fx[f"lam_x_{tag}"][i], fx[f"lam_a_{tag}"][i])
        assert max(k.values()) <= 1e-8, (i, tag, k)
    # the terrain matters: the two sets' optima differ
    assert np.max(np.abs(fx["w_A"][:, 192:] - fx["w_B"][:, 192:])) > 1.0
