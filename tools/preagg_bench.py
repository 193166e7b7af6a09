#!/usr/bin/env python3
"""Pre-aggregate generation (tsdbhip_preagg_run) beside the tsdbhip_run calls of the same
queries, on BASELINE config 2's store: 1M series x 1 h @1 s float32, 64 groups, `1m` cells in `1h`
rows, sum over each group, the four rollup functions.  One JSON line.

  preagg_ms         host wall time of one tsdbhip_preagg_run (four functions, cells left on the
                    device), median of --repeats calls after --warmup
  encode_ms         its encode stage (k_preagg_size + scan + k_preagg_write) by hipEvents
                    (tsdbhip_timing.group_reduce_ms), median; queries_ms the query passes before it
  four_runs_ms      host wall time of the four tsdbhip_run calls of the same queries (the C calls
                    alone, results assembled on the host), median, in alternation with preagg_run
  download_ms       one tsdbhip_preagg_download of the cells
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T0 = 1356998400
FUNCS = (("sum", 0), ("count", 1), ("max", 2), ("min", 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=1_000_000)
    ap.add_argument("--points", type=int, default=3600)
    ap.add_argument("--period-ms", type=int, default=1000)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--interval", default="1m")
    ap.add_argument("--span", default="1h")
    ap.add_argument("--agg", default="sum")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    args = ap.parse_args()
    from opentsdb_amd import abi, engine
    eng = engine.Engine(0)
    eng.synth(args.series, T0, args.points, args.period_ms, 0, args.groups, 2000, 0x5EED)
    eng.sync()
    iv = engine.rollup_interval(args.interval, args.span)
    start, end = T0, T0 + args.points * args.period_ms // 1000
    queries = [abi.new_query(start, end - 1, args.agg, ds_function=abi.AGG[fn], ds_interval_ms=iv.interval_s * 1000)
               for fn, _ in FUNCS]
    pre, enc, qry, runs = [], [], [], []
    cells = None
    for it in range(args.warmup + args.repeats):
        t = time.perf_counter()
        cells = eng.preagg_run(iv, start, end, args.agg, FUNCS)
        dt = (time.perf_counter() - t) * 1e3
        tm = eng.timing()
        points, dr = 0, 0.0
        for q in queries:
            res = eng.run(q)
            dr += eng.last_call_ms   # the C call alone: no Python work on the result
            points += sum(len(g[1]) for g in res)
        assert points == cells[0], (points, cells)
        if it >= args.warmup:
            pre.append(dt)
            enc.append(tm.group_reduce_ms)
            qry.append(tm.decode_downsample_ms)
            runs.append(dr)
    t = time.perf_counter()
    out = eng.preagg_download(*cells)
    dl = (time.perf_counter() - t) * 1e3
    assert len(out) == cells[0]
    med = statistics.median
    print(json.dumps({
        "bench": "preagg", "series": args.series, "points": args.points, "groups": args.groups,
        "interval": args.interval, "span": args.span, "agg": args.agg, "functions": [f for f, _ in FUNCS],
        "cells": cells[0], "qual_bytes": cells[1], "value_bytes": cells[2],
        "preagg_ms": round(med(pre), 4), "preagg_ms_min_max": [round(min(pre), 4), round(max(pre), 4)],
        "queries_ms": round(med(qry), 4), "encode_ms": round(med(enc), 4),
        "encode_share": round(med(enc) / med(pre), 5),
        "four_runs_ms": round(med(runs), 4), "four_runs_ms_min_max": [round(min(runs), 4), round(max(runs), 4)],
        "download_ms": round(dl, 4), "repeats": args.repeats, "warmup": args.warmup}))
    eng.close()


if __name__ == "__main__":
    main()
