"""bench.py helpers that need no GPU: PMC records are found by the bench's kernel label whether
rocprof's demangled name carries the interior-point template flag or not."""
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import bench  # noqa: E402


def test_counters_lookup_ignores_template_flag():
    rec_a, rec_b = {"SQ_INSTS_MFMA": 1.0}, {"SQ_INSTS_MFMA": 2.0}
    new = {"void cmpc::solve_group_kernel<192, 160, false>": rec_b,
           "void cmpc::solve_group_kernel<128, 96, false>": rec_a}
    old = {"void cmpc::solve_group_kernel<192, 160>": rec_b,
           "void cmpc::solve_group_kernel<128, 96>": rec_a}
    for c in (new, old):
        assert bench._counters_of(c, "solve_group_kernel<128, 96>") is rec_a
        assert bench._counters_of(c, "solve_group_kernel<192, 160>") is rec_b
        assert bench._counters_of(c, "solve_team_kernel<4, 1>") is None
    assert bench._counters_of(None, "solve_group_kernel<128, 96>") is None


def test_plain_run_is_headline_only_and_full_restores_the_rest():
    """Without --full every object beside the headline is off, whatever its own option says;
    --full brings back the defaults (and --full --aux 0 is headline only again)."""
    extra = ("sub_configs", "dynamics_steps", "warm_steps", "tick_steps", "leg_steps",
             "loop_steps", "api_ticks", "cpu_seconds", "scatter_steps", "weak_steps", "aux")
    for argv in (["--gpus", "1", "--steps", "7", "--warmup", "2"],
                 ["--steps", "7", "--warmup", "2", "--loop-steps", "24", "--weak-steps", "5"]):
        a = bench.parse(argv)
        assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
        assert all(getattr(a, k) == 0 for k in extra), vars(a)
    f = bench.parse(["--full", "--steps", "7"])
    assert f.full and f.aux == 1 and f.sub_configs == 1 and f.cpu_seconds == 15.0
    assert (f.dynamics_steps, f.warm_steps, f.tick_steps, f.leg_steps) == (5, 5, 5, 5)
    assert (f.loop_steps, f.api_ticks, f.scatter_steps, f.weak_steps) == (24, 20, 7, 7)
    g = bench.parse(["--full", "--aux", "0", "--weak-steps", "3"])
    assert g.sub_configs == g.loop_steps == g.cpu_seconds == g.scatter_steps == 0
    assert g.weak_steps == 3


def test_dump_outputs_writes_float32_sample(tmp_path):
    """--dump-outputs: w rows are a fixed ascending sample above the cap (all rows below it),
    every array is float32 .npy, and two dumps of the same outputs are identical."""
    import numpy as np
    cap = bench.DUMP_W_ROWS
    assert cap * 384 * 4 + 3 * 65536 * 4 <= 64 * 2 ** 20
    assert bench.dump_rows(100).tolist() == list(range(100))
    rows = bench.dump_rows(cap + 1000)
    assert len(rows) == cap and np.all(np.diff(rows) > 0) and rows[-1] < cap + 1000
    assert np.array_equal(rows, bench.dump_rows(cap + 1000))
    B = 300
    w = np.arange(B * 384, dtype=np.float32).reshape(B, 384)
    st, it = np.ones(B, np.int32), np.arange(B, dtype=np.int32)
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, w, st, it)
    got = {p.stem: np.load(p) for p in sorted((tmp_path / "a").glob("*.npy"))}
    assert sorted(got) == ["iters", "status", "w", "w_rows"]
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["w"], w) and np.array_equal(got["iters"], it)
    assert all(np.array_equal(v, np.load(tmp_path / "b" / f"{k}.npy")) for k, v in got.items())
    bench.dump_outputs(tmp_path / "r", w, st, it, rank=1, world=64)   # cap split over the ranks
    assert np.load(tmp_path / "r" / "w_rank1.npy").shape == (cap // 64, 384)


class _StubPlan:
    def __init__(self, names):
        self.names = names

    def solve_kernels(self, B):
        return list(self.names)


def _batch(n_light, n_heavy, N=16, n_mid=0):
    import numpy as np
    c = np.zeros((n_light + n_mid + n_heavy, 4, N), np.uint8)
    c[:n_light, :, :10] = 1          # 40 stance legs: 120 free forces (NC 128 bin)
    c[n_light:n_light + n_mid, :, :13] = 1  # 52 stance legs: 156 free forces (NC 160 bin)
    c[n_light + n_mid:] = 1          # 64 stance legs: 192 free forces (NC 192 bin)
    return c, np.full(n_light + n_mid + n_heavy, 8, np.int32)


def test_bins_and_kernels():
    """Five bins (NC 96 / 128 / 144 / 160 / 192) map onto the three solve kernels."""
    import numpy as np
    contact, _ = _batch(3, 2, n_mid=4)
    bins = bench.bins_of(contact)
    assert bins.tolist() == [1, 1, 1, 3, 3, 3, 3, 4, 4]
    assert bench.kernel_of_bins(np.arange(5)).tolist() == [0, 0, 1, 1, 2]


def test_roofline_dominant_and_critical_kernels():
    """Three kernels: the dominant one processes the most solves, the critical one has the
    longest live time (it sets the step); the HBM fraction is algorithmic bytes / live time."""
    contact, iters = _batch(900, 100, n_mid=50)
    bins = bench.bins_of(contact)
    plan = _StubPlan(["solve_group_kernel<128, 96, false>", "solve_group_kernel<160, 144, false>",
                      "solve_group_kernel<192, 0, false>"])
    roof, comp, crit = bench.kernel_roofline(plan, 1050, bins, contact, iters, [9.0, 4.0, 12.0],
                                             [1, 1, 1], step_ms=12.5)
    assert roof["kernel"].startswith("solve_group_kernel<128") and roof["solves_per_launch"] == 900
    assert crit["kernel"].startswith("solve_group_kernel<192") and crit["solves_per_launch"] == 100
    assert roof["solves_per_kernel"]["solve_group_kernel<160, 144, false>"] == 50
    assert not crit["same_as_dominant"] and abs(crit["step_share"] - 12.0 / 12.5) < 1e-12
    assert abs(roof["achieved"] - bench.BYTES_PER_SOLVE * 900 / 9e-3 / 1e9) < 1e-9
    assert abs(crit["frac"] - bench.BYTES_PER_SOLVE * 100 / 12e-3 / 1e9 / bench.HBM_PEAK_GBS) < 1e-12
    assert comp["kernel"] == roof["kernel"] and crit["compute"]["kernel"] == crit["kernel"]


def test_roofline_single_kernel():
    """One solve kernel for every bin (pair kernel): dominant == critical, all solves counted."""
    contact, iters = _batch(900, 100)
    plan = _StubPlan(["solve_pair_kernel<false>", None, None])
    roof, comp, crit = bench.kernel_roofline(plan, 1000, bench.bins_of(contact), contact, iters,
                                             [10.0, 0.0, 0.0], [2, 0, 0], step_ms=5.2)
    assert roof["kernel"] == crit["kernel"] == "solve_pair_kernel<false>"
    assert roof["solves_per_launch"] == 1000 and roof["kernel_avg_ms"] == 5.0
    assert crit["same_as_dominant"] and list(roof["kernel_avg_ms_all"]) == ["solve_pair_kernel<false>"]
