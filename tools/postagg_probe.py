# postagg_probe.py — times the two ways out of a finished aggregate for
#   SELECT ... GROUP BY k1, k2 ORDER BY SUM(v) DESC LIMIT 10
# on config3's query shape (about 1e6 groups at the default row count):
#   device: AggResult.to_table() + sort_topk(limit=10) + gathers of the 10 rows
#   host:   AggResult.fetch(sorted=True) + numpy top-10 (what the engine
#           offered before bkgpu_agg_to_table: download every group, finalize
#           and sort on the host)
# Each figure is the median wall time of --runs runs after --warmup runs,
# with a device sync on both sides of every run. BK_DEBUG=1 adds the engine's
# own per-stage split (permutation sort passes / finalize kernel) on stderr.
# Not bench.py, not run by any test. Prints one JSON line.
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert args.runs >= 5

    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    from baikaldb_amd import GpuEngine, QueryPlan
    from bench import CONFIGS
    cfg = CONFIGS["config3_1e9_mixed"]
    eng = GpuEngine()
    t = eng.create_table(cfg["specs"], args.rows)
    eng.generate(t, 0xC0FFEE)
    plan = QueryPlan(t.col_types, conjuncts=cfg["conjuncts"],
                     group=cfg["group"], aggs=cfg["aggs"])
    res = eng.filter_agg(t, plan, expected_groups=cfg["expected_groups"])
    ng = len(cfg["group"])
    sum_slot = ng + 1                      # SUM(c3), INT64: exact on both sides
    ncols = ng + len(cfg["aggs"])

    def gather(tab, col, ids):
        n = len(ids)
        oi, od = np.zeros(n, np.int64), np.zeros(n, np.float64)
        on = np.zeros(n, np.uint8)
        rc = eng.lib.bkgpu_gather(tab.handle, col,
                                  ids.ctypes.data_as(C.POINTER(C.c_int64)), n,
                                  oi.ctypes.data_as(C.POINTER(C.c_int64)),
                                  od.ctypes.data_as(C.POINTER(C.c_double)),
                                  on.ctypes.data_as(C.POINTER(C.c_uint8)))
        assert rc == 0
        return oi, od, on

    stages = {"to_table": [], "topk": [], "gather": []}

    def device():
        t0 = time.perf_counter()
        tab = res.to_table()
        eng.sync()
        t1 = time.perf_counter()
        ids = eng.sort_topk(tab, [(sum_slot, 0, 0)], 10)
        t2 = time.perf_counter()
        rows = [gather(tab, c, ids) for c in range(ncols)]
        t3 = time.perf_counter()
        tab.free()
        stages["to_table"].append(t1 - t0)
        stages["topk"].append(t2 - t1)
        stages["gather"].append(t3 - t2)
        return ids, rows[sum_slot][0]

    def host():
        got = res.fetch(sorted=True)
        s = got["agg_i"][1]
        # stable: ties in canonical order, like the top-N's arrival order
        ids = np.argsort(-s, kind="stable")[:10]
        return ids, s[ids]

    out = {}
    for name, fn in (("device", device), ("host", host)):
        times = []
        for i in range(args.warmup + args.runs):
            eng.sync()
            t0 = time.perf_counter()
            ids, sums = fn()
            eng.sync()
            if i >= args.warmup:
                times.append(time.perf_counter() - t0)
        out[name] = (statistics.median(times) * 1e3, ids, sums)
    assert np.array_equal(out["device"][1], out["host"][1])
    assert np.array_equal(out["device"][2], out["host"][2])
    r = args.runs
    print(json.dumps({
        "rows": args.rows, "ngroups": res.ngroups, "runs": args.runs,
        "device_ms": round(out["device"][0], 3),
        "host_fetch_ms": round(out["host"][0], 3),
        "device_stage_ms": {k: round(statistics.median(v[-r:]) * 1e3, 3)
                            for k, v in stages.items()},
    }))
    res.free()
    t.free()


if __name__ == "__main__":
    main()
