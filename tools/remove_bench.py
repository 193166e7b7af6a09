#!/usr/bin/env python3
"""tsdbhip_remove beside what the parent commit offers for a store that deletes, a tsdbhip_load of
the remaining host batch -- its stages by hipEvents, and the cost of a query step afterwards.
One JSON line a store and case.

Stores (device-synthesised, downloaded once, kept in page-locked arrays so that the load baseline
is a DMA upload): the tenths of tools/append_bench.py, tools/trim_bench.py and tools/upsert_bench.py
with three hour rows a series,
  c2   100k series x 3 x 3600 dp @1 s float32, 64 groups
  c3   1M series x 3 x 360 dp @10 s, integers / float32 alternating, 1000 groups
Cases: --what late (the middle hour's row of every 100th series goes), all (of every series), or
drop (a tenth of the series are row-less already; the call is remove([], drop_empty) alone), with
--pack 0 (TSDB_TRIM_NO_PACK) or 1 (pack_dead_pct 0).  The remaining host batch B is the download
after one call (the tests, not this tool, check that state against the oracle).

  remove_ms / load_ms    host wall time of the C call alone (the ranges are in an array built
                         beforehand), alternating in one process: load(M) (not timed), remove; then
                         load(B).  Median, min, max of --repeats after --warmup.
  stages_ms              the remove's stages by hipEvents (option TRACE, read from stderr in a pass
                         of its own): mark (the ranges' upload, k_remove_mark and the rows' way back
                         to the host), scans (the host's walk over the touched series is in it),
                         gather, suspects, pack, desc_download.
  step_*_ms              host wall time of one sum:1m-avg tsdbhip_run (the C call alone): --rounds
                         alternations of 2 warm-ups + --steps timed calls in each state -- load(M) +
                         remove against load(B); a second load(B) for the spread between two fresh
                         loads.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from append_bench import STORES, T0, pinned, stats   # noqa: E402
from trim_bench import traced   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", choices=sorted(STORES), required=True)
    ap.add_argument("--what", choices=["late", "all", "drop"], required=True)
    ap.add_argument("--pack", type=int, choices=[0, 1], default=0)
    ap.add_argument("--series", type=int, default=0, help="override the store's series count (rehearsals)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    from opentsdb_amd import abi, engine
    sp = dict(STORES[args.store])
    if args.series:
        sp["series"] = args.series
    eng = engine.Engine(0)
    L = engine.lib()
    span = sp["points"] * sp["period_ms"] // 1000
    assert span == 3600
    eng.synth(sp["series"], T0, 3 * sp["points"], sp["period_ms"], sp["value_kind"], sp["groups"], sp["int_mod"], 0x5EED)
    M = eng.download()
    n = M.n_series
    assert M.n_rows == 3 * n
    pack_pct = 0 if args.pack else abi.TRIM_NO_PACK
    flags = 0

    def range_array(idx, lo, hi):
        r = np.zeros(len(idx), dtype=[("series_index", "<i8"), ("from_s", "<i8"), ("to_s", "<i8")])
        r["series_index"], r["from_s"], r["to_s"] = idx, lo, hi
        return r

    if args.what == "drop":   # a tenth of the series lose every row first: that batch is the start
        eng.remove([(int(i), 0, 1 << 32) for i in range(0, n, 10)])
        M = eng.download()
        assert M.n_series == n and M.n_rows == 3 * (n - len(range(0, n, 10)))
        ranges = range_array(np.zeros(0, np.int64), 0, 0)
        flags = abi.REMOVE_DROP_EMPTY
    else:
        idx = np.arange(0, n, 100 if args.what == "late" else 1, dtype=np.int64)
        ranges = range_array(idx, T0 + span, T0 + 2 * span)
    M = pinned(engine, abi, M)
    info = abi.RemoveInfo()

    def remove():
        rc = L.tsdbhip_remove(eng.ctx, ranges.ctypes.data if len(ranges) else None, len(ranges), flags, pack_pct, None,
                              C.byref(info))
        assert rc == 0, rc

    eng.load(M)
    remove()
    if args.what == "drop":
        assert info.series_dropped == len(range(0, n, 10)) and info.rows_removed == 0
    else:
        assert info.rows_removed == len(ranges) and info.ranges_empty == 0
    assert info.packed == args.pack
    B = pinned(engine, abi, eng.download())
    q = abi.new_query(T0, T0 + 3 * span - 1, "sum", ds_function=abi.AGG["avg"], ds_interval_ms=60000)

    def same(r1, r2):
        assert len(r1) == len(r2)
        for (g1, t1, b1, _), (g2, t2, b2, _) in zip(r1, r2):
            assert g1 == g2 and np.array_equal(t1, t2)
            assert np.allclose(b1.view(np.float64), b2.view(np.float64), rtol=1e-9, atol=0)

    # ---- remove against load, alternating ----
    rm, ld = [], []
    for it in range(args.warmup + args.repeats):
        eng.load(M)
        eng.sync()
        t = time.perf_counter()
        remove()
        d_rm = (time.perf_counter() - t) * 1e3
        r1 = eng.run(q)
        t = time.perf_counter()
        eng.load(B)
        d_ld = (time.perf_counter() - t) * 1e3
        same(r1, eng.run(q))
        if it >= args.warmup:
            rm.append(d_rm)
            ld.append(d_ld)

    # ---- the stages, by hipEvents ----
    def five():
        for _ in range(5):
            eng.load(M)
            remove()

    st = traced(engine, five, "[trace remove]")
    # ---- the step afterwards ----
    step = {"remove": [], "load": [], "load2": []}
    for _ in range(args.rounds):
        for state in step:
            if state == "remove":
                eng.load(M)
                remove()
            else:
                eng.load(B)
            for i in range(2 + args.steps):
                eng.run(q)
                if i >= 2:
                    step[state].append(eng.last_call_ms)
    med = statistics.median
    out = {
        "bench": "remove", "store": args.store, "what": args.what, "pack": args.pack, **sp, "rows_resident": int(M.n_rows),
        "ranges": len(ranges), "rows_removed": int(info.rows_removed), "series_dropped": int(info.series_dropped),
        "remove_ms": stats(rm), "load_ms": stats(ld), "remove_over_load": round(med(rm) / med(ld), 5),
        "stages_ms": {k: stats(v) for k, v in st.items()},
        "qual_dead": int(info.qual_dead), "val_dead": int(info.val_dead),
        **{f"step_{k}_ms": stats(v) for k, v in step.items()},
        "step_ratio": round(med(step["remove"]) / med(step["load"]), 4),
        "step_load_spread": round(med(step["load2"]) / med(step["load"]), 4),
        "repeats": args.repeats, "warmup": args.warmup, "rounds": args.rounds, "steps": args.steps,
    }
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
