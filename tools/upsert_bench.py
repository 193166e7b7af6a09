#!/usr/bin/env python3
"""tsdbhip_upsert beside what the parent commit offers for a change to an old row, a tsdbhip_load
of the merged host batch -- its stages by hipEvents, and the cost of a query step afterwards.
One JSON line a store and delta.

Stores (device-synthesised, downloaded once, kept in page-locked arrays so that the load baseline
is a DMA upload): the tenths of tools/append_bench.py and tools/trim_bench.py with three hour rows
a series,
  c2   100k series x 3 x 3600 dp @1 s float32, 64 groups
  c3   1M series x 3 x 360 dp @10 s, integers / float32 alternating, 1000 groups
Deltas: the middle hour's row of --delta late (every 100th series: the late-put shape) or all
(every series: the worst case), rewritten with other values.  The merged host batch B is the
download after one upsert (the tests, not this tool, check that state against the oracle).

  upsert_ms / load_ms    host wall time of one call, alternating in one process: load(M) (not
                         timed), upsert(D); then load(B).  Median, min, max of --repeats after
                         --warmup.
  stages_ms              the upsert's stages by hipEvents (option TRACE, read from stderr in a
                         pass of its own): grow_copy, upload, index_rank (the delta's index pass
                         and k_upsert_rank; delta_index is the pass alone), hit_scan, rank_download
                         (the ranks' way to the host and the host's pass over them), scan_gather,
                         suspects (suspect_index: their index pass alone), recede, desc_download.
  step_*_ms              host wall time of one sum:1m-avg tsdbhip_run (the C call alone): --rounds
                         alternations of 2 warm-ups + --steps timed calls in each state -- load(M) +
                         upsert(D) against load(B); a second load(B) for the spread between two
                         fresh loads.
"""
from __future__ import annotations

import argparse
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


def subset(abi, b, idx):
    """The one-row-a-series batch `b` restricted to series idx."""
    assert b.n_rows == b.n_series
    qo, vo = b.row_qual_off.astype(np.int64), b.row_val_off.astype(np.int64)
    if len(idx) == b.n_series:
        return b

    def blob(off, data):
        lens = np.diff(off)[idx]
        out = np.zeros(len(idx) + 1, np.int64)
        out[1:] = np.cumsum(lens)
        pos = np.repeat(off[:-1][idx] - out[:-1], lens) + np.arange(int(out[-1]), dtype=np.int64)
        return out.astype(np.uint64), data[pos]

    nqo, nq = blob(qo, b.qual)
    nvo, nv = blob(vo, b.val)
    return abi.HostBatch(np.arange(len(idx) + 1, dtype=np.int64), b.row_base_time[:b.n_rows][idx], nqo, nvo, nq, nv,
                         b.group_id[idx])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", choices=sorted(STORES), required=True)
    ap.add_argument("--delta", choices=["late", "all"], required=True)
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
    span = sp["points"] * sp["period_ms"] // 1000
    assert span == 3600
    eng.synth(sp["series"], T0 + span, sp["points"], sp["period_ms"], sp["value_kind"], sp["groups"], sp["int_mod"], 0xBEEF)
    hour = eng.download()                                  # the middle hour as the store holds it now
    n = hour.n_series
    idx = np.arange(0, n, 100 if args.delta == "late" else 1, dtype=np.int64)
    D = pinned(engine, abi, subset(abi, hour, idx))
    del hour
    eng.synth(sp["series"], T0, 3 * sp["points"], sp["period_ms"], sp["value_kind"], sp["groups"], sp["int_mod"], 0x5EED)
    M = pinned(engine, abi, eng.download())
    assert M.n_series == n and M.n_rows == 3 * n
    zeros = np.zeros(len(idx), np.uint8)
    info = eng.upsert(D, idx, zeros)
    assert (info.series_added, info.rows_added, info.rows_replaced) == (0, 0, len(idx))
    B = pinned(engine, abi, eng.download())
    assert B.n_rows == 3 * n
    q = abi.new_query(T0, T0 + 3 * span - 1, "sum", ds_function=abi.AGG["avg"], ds_interval_ms=60000)

    def same(r1, r2):
        assert len(r1) == len(r2) == sp["groups"]
        for (g1, t1, b1, _), (g2, t2, b2, _) in zip(r1, r2):
            assert g1 == g2 and np.array_equal(t1, t2)
            assert np.allclose(b1.view(np.float64), b2.view(np.float64), rtol=1e-9, atol=0)

    # ---- upsert against load, alternating ----
    up, ld = [], []
    for it in range(args.warmup + args.repeats):
        eng.load(M)
        eng.sync()
        t = time.perf_counter()
        info = eng.upsert(D, idx, zeros)
        d_up = (time.perf_counter() - t) * 1e3
        r1 = eng.run(q)
        t = time.perf_counter()
        eng.load(B)
        d_ld = (time.perf_counter() - t) * 1e3
        same(r1, eng.run(q))
        if it >= args.warmup:
            up.append(d_up)
            ld.append(d_ld)

    # ---- the stages, by hipEvents ----
    def five():
        for _ in range(5):
            eng.load(M)
            eng.upsert(D, idx, zeros)

    st = traced(engine, five, "[trace upsert]")
    # ---- the step afterwards ----
    step = {"upsert": [], "load": [], "load2": []}
    for _ in range(args.rounds):
        for state in step:
            if state == "upsert":
                eng.load(M)
                eng.upsert(D, idx, zeros)
            else:
                eng.load(B)
            for i in range(2 + args.steps):
                eng.run(q)
                if i >= 2:
                    step[state].append(eng.last_call_ms)
    med = statistics.median
    out = {
        "bench": "upsert", "store": args.store, "delta": args.delta, **sp, "rows_resident": 3 * n, "rows_replaced": len(idx),
        "delta_cell_bytes": int(D.row_qual_off[-1] + D.row_val_off[-1]),
        "upsert_ms": stats(up), "load_ms": stats(ld), "upsert_over_load": round(med(up) / med(ld), 5),
        "stages_ms": {k: stats(v) for k, v in st.items()},
        "grew": int(info.grew), "qual_dead": int(info.qual_dead), "val_dead": int(info.val_dead),
        **{f"step_{k}_ms": stats(v) for k, v in step.items()},
        "step_ratio": round(med(step["upsert"]) / med(step["load"]), 4),
        "step_load_spread": round(med(step["load2"]) / med(step["load"]), 4),
        "repeats": args.repeats, "warmup": args.warmup, "rounds": args.rounds, "steps": args.steps,
    }
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
