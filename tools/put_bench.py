#!/usr/bin/env python3
"""tsdbhip_put beside what the parent commit offers for the same change, a tsdbhip_upsert of the
rewritten rows from page-locked arrays -- its stages by hipEvents, k_put's bytes a second, and the
cost of a query step afterwards.  One JSON line a store and shape.

Stores (device-synthesised, downloaded once, kept in page-locked arrays): the tenths of
tools/upsert_bench.py with three hour rows a series,
  c2   100k series x 3 x 3600 dp @1 s float32, 64 groups
  c3   1M series x 3 x 360 dp @10 s, integers / float32 alternating, 1000 groups
Shapes: --shape late (every 100th series, one point in the middle of the middle hour's row: the
walked route) or tick (every series, one point behind the last hour's last datapoint: the tail
route).  On c2 every second is taken, so the points are millisecond points.  The rewritten rows D
are the touched rows of the download after one put (the tests, not this tool, check that state
against the oracle).

  put_ms / upsert_ms     host wall time of one call, alternating in one process: load(M) (not
                         timed), put(P); load(M) (not timed), upsert(D); which of the two comes
                         first swaps every iteration (--order fixed: the put always first).
                         Median, min, max of --repeats after --warmup.
  kernel_ms              tsdbhip_put_info.kernel_ms (hipEvents around k_put) of the timed calls;
                         copy_fraction: k_put's bytes moved -- the rewritten cells read and
                         written -- over kernel_ms, as a fraction of the 6.29 TB/s float4-copy rate.
  stages_ms              the put's stages by hipEvents (option TRACE, read from stderr in a pass
                         of its own), named as tools/upsert_bench.py names the upsert's; `upload`
                         is the slots' zeroing, the puts' upload and k_put.
  step_*_ms              host wall time of one sum:1m-avg tsdbhip_run: --rounds alternations of 2
                         warm-ups + --steps timed calls in each state -- load(M) + put(P) against
                         load(B); a second load(B) for the spread between two fresh loads.
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

COPY_RATE = 6.29e12   # bytes a second, the float4 copy of DESIGN.md 7


def rows_subset(abi, b, rows, gids):
    """One row a series: rows `rows` of batch `b`."""
    qo, vo = b.row_qual_off.astype(np.int64), b.row_val_off.astype(np.int64)

    def blob(off, data):
        lens = np.diff(off)[rows]
        out = np.zeros(len(rows) + 1, np.int64)
        out[1:] = np.cumsum(lens)
        pos = np.repeat(off[:-1][rows] - out[:-1], lens) + np.arange(int(out[-1]), dtype=np.int64)
        return out.astype(np.uint64), data[pos]

    nqo, nq = blob(qo, b.qual)
    nvo, nv = blob(vo, b.val)
    return abi.HostBatch(np.arange(len(rows) + 1, dtype=np.int64), b.row_base_time[:b.n_rows][rows], nqo, nvo, nq, nv,
                         np.asarray(gids, np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", choices=sorted(STORES), required=True)
    ap.add_argument("--shape", choices=["late", "tick"], required=True)
    ap.add_argument("--series", type=int, default=0, help="override the store's series count (rehearsals)")
    ap.add_argument("--order", choices=["swap", "fixed"], default="swap", help="which of the two timed calls comes first")
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
    eng.synth(sp["series"], T0, 3 * sp["points"], sp["period_ms"], sp["value_kind"], sp["groups"], sp["int_mod"], 0x5EED)
    M = pinned(engine, abi, eng.download())
    n = M.n_series
    assert M.n_rows == 3 * n
    # the points: between two datapoints of the middle hour, or behind the last datapoint of the last hour
    idx = np.arange(0, n, 100 if args.shape == "late" else 1, dtype=np.int64)
    half = sp["period_ms"] // 2
    hour = 1 if args.shape == "late" else 2
    at_ms = (T0 + hour * span) * 1000 + ((sp["points"] // 2) if args.shape == "late" else (sp["points"] - 1)) * sp["period_ms"] + half
    P = np.zeros(len(idx), abi.POINT_DTYPE)
    P["series_index"] = idx
    P["timestamp"] = at_ms if at_ms % 1000 else at_ms // 1000
    P["kind"] = abi.PUT_FLOAT
    P["bits"] = np.float32(0.25 * (1 + idx % 64)).view(np.uint32)
    info = eng.put(P)
    # (a tick takes the tail route where the resident row has one value length; c3's integer rows vary)
    assert info.rows_added == 0 and info.rows_walked + info.rows_tail == len(idx), (info.rows_added, info.rows_walked, info.rows_tail)
    assert info.rows_tail == 0 if args.shape == "late" else info.rows_tail > 0
    B = pinned(engine, abi, eng.download())
    assert B.n_rows == 3 * n
    rows = idx * 3 + hour
    D = pinned(engine, abi, rows_subset(abi, B, rows, B.group_id[idx]))
    moved = 2 * int(D.row_qual_off[-1] + D.row_val_off[-1])   # k_put reads the resident cells and writes the merged ones
    zeros = np.zeros(len(idx), np.uint8)
    q = abi.new_query(T0, T0 + 3 * span - 1, "sum", ds_function=abi.AGG["avg"], ds_interval_ms=60000)

    def same(r1, r2):
        assert len(r1) == len(r2) == sp["groups"]
        for (g1, t1, b1, _), (g2, t2, b2, _) in zip(r1, r2):
            assert g1 == g2 and np.array_equal(t1, t2)
            assert np.allclose(b1.view(np.float64), b2.view(np.float64), rtol=1e-9, atol=0)

    # ---- put against upsert, alternating ----
    put, ups, kms = [], [], []

    def timed_put():
        eng.load(M)
        eng.sync()
        t = time.perf_counter()
        info = eng.put(P)
        return (time.perf_counter() - t) * 1e3, info, eng.run(q)

    def timed_upsert():
        eng.load(M)
        eng.sync()
        t = time.perf_counter()
        eng.upsert(D, idx, zeros)
        return (time.perf_counter() - t) * 1e3, eng.run(q)

    for it in range(args.warmup + args.repeats):
        # (which call comes first swaps every iteration, so that neither call always follows the load
        # that released the other's grown blobs)
        if args.order == "fixed" or it % 2 == 0:
            d_put, info, r1 = timed_put()
            d_up, r2 = timed_upsert()
        else:
            d_up, r2 = timed_upsert()
            d_put, info, r1 = timed_put()
        same(r1, r2)
        if it >= args.warmup:
            put.append(d_put)
            ups.append(d_up)
            kms.append(info.kernel_ms)

    # ---- the stages, by hipEvents ----
    def five():
        for _ in range(5):
            eng.load(M)
            eng.put(P)

    st = traced(engine, five, "[trace put] (upload: the slots zeroed and k_put) [trace upsert]")
    host = traced(engine, five, "[trace put] points")     # host_prep: validation and buckets; build: the puts' upload, k_put, the report
    # ---- the step afterwards ----
    step = {"put": [], "load": [], "load2": []}
    for _ in range(args.rounds):
        for state in step:
            if state == "put":
                eng.load(M)
                eng.put(P)
            else:
                eng.load(B)
            for i in range(2 + args.steps):
                eng.run(q)
                if i >= 2:
                    step[state].append(eng.last_call_ms)
    med = statistics.median
    out = {
        "bench": "put", "store": args.store, "shape": args.shape, **sp, "rows_resident": 3 * n, "points": len(idx),
        "point_bytes": int(P.nbytes), "rewritten_cell_bytes": int(D.row_qual_off[-1] + D.row_val_off[-1]),
        "put_ms": stats(put), "upsert_ms": stats(ups), "put_over_upsert": round(med(put) / med(ups), 5),
        "kernel_ms": stats(kms), "k_put_bytes_moved": moved,
        "copy_fraction": round(moved / (med(kms) * 1e-3) / COPY_RATE, 4),
        "stages_ms": {k: stats(v) for k, v in st.items()},
        "put_host_ms": {k: stats(v) for k, v in host.items() if k in ("host_prep", "build", "call")},
        "rows_tail": int(info.rows_tail), "rows_walked": int(info.rows_walked),
        "grew": int(info.grew), "qual_dead": int(info.qual_dead), "val_dead": int(info.val_dead),
        **{f"step_{k}_ms": stats(v) for k, v in step.items()},
        "step_ratio": round(med(step["put"]) / med(step["load"]), 4),
        "step_load_spread": round(med(step["load2"]) / med(step["load"]), 4),
        "order": args.order, "repeats": args.repeats, "warmup": args.warmup, "rounds": args.rounds, "steps": args.steps,
    }
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
