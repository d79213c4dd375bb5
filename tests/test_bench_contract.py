# Guards the bench.py driver contract: config shapes stay self-consistent
# (column references valid, analytic byte counts sane, wire-blob size math
# matches the engine's export layout).
import json
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_configs_self_consistent():
    import bench
    for name, cfg in bench.CONFIGS.items():
        ncols = len(cfg["specs"])
        for col, _op, _lit in cfg["conjuncts"]:
            assert 0 <= col < ncols, (name, col)
        for col in cfg["group"]:
            assert 0 <= col < ncols, (name, col)
        for _fn, col in cfg["aggs"]:
            assert col == -1 or 0 <= col < ncols, (name, col)
        for col, _asc, _nf in cfg.get("order", ()):
            assert 0 <= col < ncols, (name, col)
        assert 0 < cfg["bytes_per_row"] <= 8 * ncols + 1, name
        assert len(cfg["group"]) <= 4 and len(cfg["aggs"]) <= 8, name


def test_wire_blob_per_group_math():
    """bench.one_step sizes peer blobs analytically as 20 + 16*naggs; the
    header documents [flags u32][k0 u64][k1 u64][states u64*2*naggs] — keep
    the two in sync (include/bkgpu.h wire format)."""
    hdr = open(os.path.join(REPO, "include", "bkgpu.h")).read()
    assert "[ flags: u32 * n ][ k0: u64 * n ][ k1: u64 * n ]" in hdr
    # 4 + 8 + 8 + 16*naggs == 20 + 16*naggs
    src = open(os.path.join(REPO, "bench.py")).read()
    assert "per_group = 20 + 16 * len(cfg[\"aggs\"])" in src


class _FakeAggResult:
    """Stands in for AggResult.fetch(): n groups in canonical order."""

    def __init__(self, n, na):
        import numpy as np
        g = np.arange(n, dtype=np.uint64)
        enc = np.zeros((n, 4), dtype=np.uint64)
        enc[:, 0] = (np.uint64(1) << np.uint64(63)) | g   # sign-flipped key
        enc[:, 1] = g * np.uint64(3)
        self.got = {"ngroups": n, "rows_passed": 7 * n,
                    "flags": np.zeros(n, np.uint8), "enc": enc,
                    "agg_i": np.arange(na * n, dtype=np.int64).reshape(na, n),
                    "agg_d": np.full((na, n), 0.5),
                    "agg_has": np.ones((na, n), np.uint8)}

    def fetch(self, sorted=True):
        assert sorted
        return self.got


def test_dump_outputs_float64_exact_keys_and_bounded(tmp_path):
    """--dump-outputs: every array lands as float64 .npy, u64 keys survive as
    exact halves, each aggregate comes from its own lane, and a result past
    the budget is cut to the same seeded sample on every run."""
    import numpy as np
    import bench
    cfg = bench.CONFIGS["config3_1e9_mixed"]
    na = len(cfg["aggs"])

    small = bench.agg_outputs(_FakeAggResult(1000, na), cfg)
    bench.dump_outputs(str(tmp_path), small)
    back = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(back) == set(small)
    assert all(a.dtype == np.float64 for a in back.values())
    assert np.array_equal(back["group_index"], np.arange(1000))
    key0 = back["key_hi"][:, 0] * 2.0**32 + back["key_lo"][:, 0]
    assert np.array_equal(back["key_hi"][:, 0], np.full(1000, 2.0**31))
    assert np.array_equal(back["key_lo"][:, 0], np.arange(1000))
    assert key0[5] == 2.0**63 + 5
    assert back["key_hi"].shape == (1000, len(cfg["group"]))
    # count_star and SUM(int64) from the int lane, SUM/AVG(double) from the other
    assert np.array_equal(back["agg"][1], np.arange(1000, 2000))
    assert np.array_equal(back["agg"][2], np.full(1000, 0.5))
    assert back["ngroups"][0] == 1000 and back["rows_passed"][0] == 7000

    n = 1_000_000
    big1 = bench.agg_outputs(_FakeAggResult(n, na), cfg)
    big2 = bench.agg_outputs(_FakeAggResult(n, na), cfg)
    m = len(big1["group_index"])
    assert 0 < m < n and np.array_equal(big1["group_index"], big2["group_index"])
    assert np.all(np.diff(big1["group_index"]) > 0)
    assert np.array_equal(big1["agg"][0], big1["group_index"])
    total = sum(np.asarray(a).size * 8 for a in big1.values())
    assert total <= 64 * 10**6


def test_plain_run_skips_cpu_baseline_leg():
    """The CPU baseline runs only behind --full."""
    src = open(os.path.join(REPO, "bench.py")).read()
    assert "if args.full and n_gpus == 1 and not args.no_cpu_baseline:" in src
    assert "setperflevel" not in src


def test_baseline_metric_matches_bench():
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))
    src = open(os.path.join(REPO, "bench.py")).read()
    assert "config3_1e9_mixed" in src
    assert base.get("metric") is None or "rows" in str(base.get("metric", ""))
