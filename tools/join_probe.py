#!/usr/bin/env python3
"""Join probe: fact-to-dimension INNER join, both probe routes, per stage.

Outer side: --rows rows x 3 INT64 columns (wide storage), key uniform so
that about 90% of the rows find a match. Inner sides: 1e3 / 1e4 / 1e5 / 1e6
unique keys x 2 payload columns. Output: the key and one payload column from
each side.

Protocol: per inner size, 2 warm-ups then 7 timed runs; every run joins once
with BK_JOIN_LDS_KB=0 (slots probed in HBM/L2) and once with
BK_JOIN_LDS_KB=<--lds-kb> (slots copied to LDS where they fit), alternating in
the same process, the device synchronised on both sides of each join. Stage
times are the engine's HIP-event times (join_stats). Reported: the median per
stage and route, the run-to-run spread of count+emit on the global route
((max - min) / median), and the achieved bytes/s of count+emit against the
algorithmic bytes computed here from the shapes: the outer key column read
twice plus the pair list written.

Prints one JSON line per inner size and a summary table.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

I64 = 6
STAGES = ("build", "count", "emit", "gather")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--inner", type=int, nargs="+",
                    default=[1_000, 10_000, 100_000, 1_000_000])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lds-kb", type=int, default=128)
    ap.add_argument("--seed", type=int, default=20240611)
    args = ap.parse_args()

    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    from baikaldb_amd import GpuEngine
    eng = GpuEngine()
    rng = np.random.default_rng(args.seed)
    rows = []
    for k in args.inner:
        span = int(round(k / 0.9))            # ~90% of outer keys are present
        outer = eng.create_table([(I64, 0, 0, span, 0), (I64, 0, 0, 1 << 40, 0),
                                  (I64, 0, 0, 1000, 0)], args.rows)
        eng.generate(outer, args.seed + k, compact=False)
        inner = eng.create_table([(I64, 0, 0, 0, 0)] * 3, k)
        eng.upload(inner, 0, rng.permutation(k).astype(np.int64))
        eng.upload(inner, 1, rng.integers(0, 1 << 40, k))
        eng.upload(inner, 2, rng.integers(0, 1000, k))
        out = [(0, 0), (0, 1), (1, 1)]         # key + one payload per side
        knobs = {"global": "0", "lds": str(args.lds_kb)}
        ms = {r: {s: [] for s in STAGES} for r in knobs}
        took, nrows, tbytes = {}, 0, 0
        for it in range(args.warmup + args.runs):
            for route, kb in knobs.items():
                os.environ["BK_JOIN_LDS_KB"] = kb
                eng.sync()
                res = eng.join(outer, inner, [(0, 0)], "inner", out=out)
                eng.sync()
                st = eng.join_stats()
                res.free()
                took[route], nrows, tbytes = st["route"], st["rows"], st["table_bytes"]
                if it >= args.warmup:
                    for s in STAGES:
                        ms[route][s].append(st["stage_ms"][s])
        os.environ.pop("BK_JOIN_LDS_KB", None)
        outer.free()
        inner.free()
        eng.lib.bkgpu_pool_trim()
        # algorithmic bytes of count + emit, from the shapes
        algo = 2 * args.rows * 8 + nrows * 8
        rec = {"outer_rows": args.rows, "inner_keys": k, "result_rows": nrows,
               "table_bytes": tbytes, "algo_bytes_count_emit": algo}
        for route in knobs:
            med = {s: statistics.median(ms[route][s]) for s in STAGES}
            probe = [c + e for c, e in zip(ms[route]["count"], ms[route]["emit"])]
            pmed = statistics.median(probe)
            rec[route] = {"route_taken": took[route],
                          "median_ms": {s: round(v, 4) for s, v in med.items()},
                          "count_emit_ms": round(pmed, 4),
                          "count_emit_spread": round((max(probe) - min(probe)) / pmed, 4),
                          "count_emit_GBps": round(algo / pmed / 1e6, 1)}
        rows.append(rec)
        print(json.dumps(rec), flush=True)

    print("\ninner keys | table KB | route  | build | count | emit | gather | "
          "count+emit ms | spread | GB/s")
    for r in rows:
        for route in ("global", "lds"):
            x = r[route]
            m = x["median_ms"]
            print(f"{r['inner_keys']:>10} | {r['table_bytes'] / 1024:>8.0f} | "
                  f"{x['route_taken']:<6} | {m['build']:.3f} | {m['count']:.3f} | "
                  f"{m['emit']:.3f} | {m['gather']:.3f} | "
                  f"{x['count_emit_ms']:.3f} | {x['count_emit_spread']:.3f} | "
                  f"{x['count_emit_GBps']:.0f}")


if __name__ == "__main__":
    main()
