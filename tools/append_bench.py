#!/usr/bin/env python3
"""tsdbhip_append beside the only other way to extend a resident store, a tsdbhip_load of the
merged host batch -- and the cost of a query step afterwards.  One JSON line a store.

Stores (device-synthesised, downloaded once, kept in page-locked arrays so that the load baseline
is a DMA upload): the tenths of tools/regroup_bench.py,
  c2   100k series x 3600 dp @1 s float32, 64 groups
  c3   1M series x 360 dp @10 s, integers / float32 alternating, 1000 groups
A is the store's hour [T0, T0 + 1 h): one row a series, the live row.  The delta D holds, for
every series, that row again (a replacement) and the row of the next hour; the merged batch M has
two rows a series.

  append_ms / load_ms    host wall time of one call, alternating in one process: load(A) (not
                         timed), append(D), then load(M).  Median, min, max of --repeats after
                         --warmup.  append_ms is the first append onto an exact-fit load, so it
                         includes the growth copy.
  append_nogrow_ms       the same delta's rows replaced once more (every series' two last rows
                         cannot both be replaced, so: the next-hour row alone, replaced in place)
                         with room left by the first append: no re-allocation.
  stages_ms              the append's stages by hipEvents (option TRACE, read from stderr in a
                         pass of its own): grow_copy, upload, index, scan_gather, desc_download.
  step_append_ms /       host wall time of one sum:1m-avg tsdbhip_run (the C call alone) after
  step_load_ms           load(A) + append(D) / after load(M): --rounds alternations of 2 warm-ups
                         + --steps timed calls in each state.  step_load2_ms: a second fresh load
                         in the same alternation, for the spread between two fresh loads.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T0 = 1356998400
STORES = {
    "c2": dict(series=100_000, points=3600, period_ms=1000, value_kind=0, groups=64, int_mod=2000),
    "c3": dict(series=1_000_000, points=360, period_ms=10000, value_kind=2, groups=1000, int_mod=30000),
}


def stats(x):
    return {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4)}


def pinned(engine, abi, b):
    return abi.HostBatch(*[engine.pinned_copy(a) for a in (b.series_row_ptr, b.row_base_time, b.row_qual_off,
                                                           b.row_val_off, b.qual, b.val, b.group_id)])


def interleave(a, b):
    """The batch with, for every series, its row of `a` and then its row of `b` (one row a series each)."""
    from opentsdb_amd import abi
    n = a.n_series
    assert a.n_rows == n and b.n_rows == n

    def blob(ao, bo, ab, bb):
        la, lb = np.diff(ao.astype(np.int64)), np.diff(bo.astype(np.int64))
        lens = np.stack([la, lb], axis=1).ravel()
        off = np.zeros(2 * n + 1, np.int64)
        off[1:] = np.cumsum(lens)
        out = np.empty(int(off[-1]), np.uint8)
        if len(set(la.tolist())) == 1 and len(set(lb.tolist())) == 1:   # uniform rows: one reshape
            m = out.reshape(n, int(la[0] + lb[0]))
            m[:, :la[0]] = ab[:int(ao[n])].reshape(n, la[0])
            m[:, la[0]:] = bb[:int(bo[n])].reshape(n, lb[0])
        else:
            for src_off, src, col in ((ao.astype(np.int64), ab, 0), (bo.astype(np.int64), bb, 1)):
                for s0 in range(0, n, 32768):   # (a byte-index gather, in chunks that bound its int64 indices)
                    s1 = min(n, s0 + 32768)
                    ln = np.diff(src_off[s0:s1 + 1])
                    tot = int(src_off[s1] - src_off[s0])
                    rel = np.arange(tot, dtype=np.int64) - np.repeat(src_off[s0:s1] - src_off[s0], ln)
                    out[np.repeat(off[2 * s0 + col:2 * s1 + col:2], ln) + rel] = src[int(src_off[s0]):int(src_off[s1])]
        return off.astype(np.uint64), out

    qo, q = blob(a.row_qual_off, b.row_qual_off, a.qual, b.qual)
    vo, v = blob(a.row_val_off, b.row_val_off, a.val, b.val)
    base = np.stack([a.row_base_time[:n], b.row_base_time[:n]], axis=1).ravel()
    return abi.HostBatch(np.arange(n + 1, dtype=np.int64) * 2, base, qo, vo, q, v, a.group_id)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", choices=sorted(STORES), required=True)
    ap.add_argument("--series", type=int, default=0, help="override the store's series count (rehearsals)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
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
    eng.synth(sp["series"], T0, sp["points"], sp["period_ms"], sp["value_kind"], sp["groups"], sp["int_mod"], 0x5EED)
    a = eng.download()
    eng.synth(sp["series"], T0 + span, sp["points"], sp["period_ms"], sp["value_kind"], sp["groups"], sp["int_mod"], 0x5EED)
    b = eng.download()
    n = a.n_series
    m = interleave(a, b)
    A, M, B = pinned(engine, abi, a), pinned(engine, abi, m), pinned(engine, abi, b)
    D = M   # the live row again and the next hour's row, for every series
    del a, b, m
    idx, new = np.arange(n, dtype=np.int64), np.zeros(n, np.uint8)
    q = abi.new_query(T0, T0 + 2 * span - 1, "sum", ds_function=abi.AGG["avg"], ds_interval_ms=60000)

    def same(r1, r2):
        assert len(r1) == len(r2) == sp["groups"]
        for (g1, t1, b1, _), (g2, t2, b2, _) in zip(r1, r2):
            assert g1 == g2 and np.array_equal(t1, t2)
            assert np.allclose(b1.view(np.float64), b2.view(np.float64), rtol=1e-9, atol=0)

    # ---- append against load, alternating ----
    apd, ld, nog = [], [], []
    info = None
    for it in range(args.warmup + args.repeats):
        eng.load(A)
        eng.sync()
        t = time.perf_counter()
        info = eng.append(D, idx, new)
        d_ap = (time.perf_counter() - t) * 1e3
        assert (info.rows_added, info.rows_replaced, info.grew) == (n, n, 1)
        r1 = eng.run(q)
        t = time.perf_counter()
        i2 = eng.append(B, idx, new)     # the next-hour row replaced in the room the first append left
        d_ng = (time.perf_counter() - t) * 1e3
        assert (i2.rows_added, i2.rows_replaced, i2.grew) == (0, n, 0)
        t = time.perf_counter()
        eng.load(M)
        d_ld = (time.perf_counter() - t) * 1e3
        same(r1, eng.run(q))
        if it >= args.warmup:
            apd.append(d_ap)
            ld.append(d_ld)
            nog.append(d_ng)
    # ---- the stages, by hipEvents (option TRACE writes them to stderr) ----
    stages = {}
    with tempfile.TemporaryFile() as tf:
        saved = os.dup(2)
        try:
            for _ in range(5):
                eng.load(A)
                sys.stderr.flush()
                os.dup2(tf.fileno(), 2)
                with engine.options(TRACE=1):
                    eng.append(D, idx, new)
                os.dup2(saved, 2)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tf.seek(0)
        for ln in tf.read().decode(errors="replace").splitlines():
            if ln.startswith("[trace append]"):
                for k, v in re.findall(r"(\w+) ([0-9.]+)", ln[len("[trace append]"):]):
                    stages.setdefault(k, []).append(float(v))
    # ---- the step afterwards ----
    step = {"append": [], "load": [], "load2": []}
    for _ in range(args.rounds):
        for state in ("append", "load", "load2"):
            if state == "append":
                eng.load(A)
                eng.append(D, idx, new)
            else:
                eng.load(M)
            for i in range(2 + args.steps):
                eng.run(q)
                if i >= 2:
                    step[state].append(eng.last_call_ms)
    med = statistics.median
    out = {
        "bench": "append", "store": args.store, **sp, "rows_resident": n, "rows_delta": 2 * n,
        "delta_cell_bytes": int(D.qual.nbytes + D.val.nbytes), "merged_cell_bytes": int(M.qual.nbytes + M.val.nbytes),
        "append_ms": stats(apd), "append_nogrow_ms": stats(nog), "load_ms": stats(ld),
        "append_over_load": round(med(apd) / med(ld), 5),
        "stages_ms": {k: stats(v) for k, v in stages.items()},
        "qual_capacity": int(info.qual_capacity), "val_capacity": int(info.val_capacity),
        "step_append_ms": stats(step["append"]), "step_load_ms": stats(step["load"]), "step_load2_ms": stats(step["load2"]),
        "step_ratio": round(med(step["append"]) / med(step["load"]), 4),
        "step_load_spread": round(med(step["load2"]) / med(step["load"]), 4),
        "repeats": args.repeats, "warmup": args.warmup, "rounds": args.rounds, "steps": args.steps,
    }
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
