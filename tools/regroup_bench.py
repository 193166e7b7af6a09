#!/usr/bin/env python3
"""tsdbhip_regroup beside the only other way to change the grouping of a resident store, a
tsdbhip_load of the same host batch with the new ids -- and the cost of a query step afterwards.
One JSON line a store.

Stores (device-synthesised, downloaded once, kept in page-locked arrays so the load baseline is a
DMA upload):
  c2   a tenth of BASELINE config 2: 100k series x 3600 dp @1 s float32, 64 groups
  c3   a tenth of BASELINE config 3: 1M series x 360 dp @10 s, integers / float32 alternating,
       1000 groups
Groupings: A, the store's own (series sorted by group); B, a hash of the batch position over the
same number of groups, so that every tile's series are scattered over the blobs.

  regroup_ms / load_ms   host wall time of one call, alternating in one process: iteration i
                         regroups to (B, A, B, ...) and then loads the host batch with the same
                         ids.  Median, min, max of --repeats after --warmup.
  step_regroup_ms /      host wall time of one sum:1m-avg tsdbhip_run (the C call alone) on
  step_load_ms           grouping B reached by load(A) + regroup(B) / by load(B): --rounds
                         alternations of 2 warm-ups + --steps timed calls in each state.
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

T0 = 1356998400
STORES = {
    "c2": dict(series=100_000, points=3600, period_ms=1000, value_kind=0, groups=64, int_mod=2000),
    "c3": dict(series=1_000_000, points=360, period_ms=10000, value_kind=2, groups=1000, int_mod=30000),
}


def stats(x):
    return {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4)}


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
    eng.synth(sp["series"], T0, sp["points"], sp["period_ms"], sp["value_kind"], sp["groups"], sp["int_mod"], 0x5EED)
    t = time.perf_counter()
    host = eng.download()
    download_s = time.perf_counter() - t
    n = host.n_series
    arrays = [engine.pinned_copy(a) for a in (host.series_row_ptr, host.row_base_time, host.row_qual_off,
                                              host.row_val_off, host.qual, host.val)]
    ids_a = host.group_id.copy()
    ids_b = ((np.arange(n, dtype=np.int64) * 2654435761 >> 7) % sp["groups"]).astype(np.int32)
    batch = {"A": abi.HostBatch(*arrays, engine.pinned_copy(ids_a)), "B": abi.HostBatch(*arrays, engine.pinned_copy(ids_b))}
    ids = {"A": ids_a, "B": ids_b}
    del host
    end = T0 + sp["points"] * sp["period_ms"] // 1000
    q = abi.new_query(T0, end - 1, "sum", ds_function=abi.AGG["avg"], ds_interval_ms=60000)

    def points(res):
        return sum(len(g[1]) for g in res)

    # ---- regroup against load, alternating ----
    eng.load(batch["A"])
    rg, ld = [], []
    for it in range(args.warmup + args.repeats):
        k = "B" if it % 2 == 0 else "A"
        t = time.perf_counter()
        eng.regroup(ids[k])
        d_rg = (time.perf_counter() - t) * 1e3
        r1 = eng.run(q)
        t = time.perf_counter()
        eng.load(batch[k])
        d_ld = (time.perf_counter() - t) * 1e3
        r2 = eng.run(q)
        assert len(r1) == len(r2) == sp["groups"] and points(r1) == points(r2)
        for (g1, t1, b1, _), (g2, t2, b2, _) in zip(r1, r2):
            assert g1 == g2 and np.array_equal(t1, t2)
            assert np.allclose(b1.view(np.float64), b2.view(np.float64), rtol=1e-9, atol=0)
        if it >= args.warmup:
            rg.append(d_rg)
            ld.append(d_ld)
    # ---- the step afterwards ----
    step = {"regroup": [], "load": []}
    for _ in range(args.rounds):
        for state in ("regroup", "load"):
            if state == "regroup":
                eng.load(batch["A"])
                eng.regroup(ids["B"])
            else:
                eng.load(batch["B"])
            for i in range(2 + args.steps):
                eng.run(q)
                if i >= 2:
                    step[state].append(eng.last_call_ms)
    ns, nr = eng.n_series(), host_rows(eng)
    out = {
        "bench": "regroup", "store": args.store, **sp, "rows": nr, "download_s": round(download_s, 2),
        "cell_bytes": int(arrays[4].nbytes + arrays[5].nbytes), "descriptor_bytes": 48 * nr,
        "regroup_ms": stats(rg), "load_ms": stats(ld),
        "regroup_over_load": round(statistics.median(rg) / statistics.median(ld), 5),
        "step_regroup_ms": stats(step["regroup"]), "step_load_ms": stats(step["load"]),
        "step_ratio": round(statistics.median(step["regroup"]) / statistics.median(step["load"]), 4),
        "repeats": args.repeats, "warmup": args.warmup, "rounds": args.rounds, "steps": args.steps,
    }
    assert ns == n
    print(json.dumps(out))
    eng.close()


def host_rows(eng):
    import ctypes as C
    from opentsdb_amd import engine
    ns, nr, qb, vb = C.c_int64(), C.c_int64(), C.c_uint64(), C.c_uint64()
    engine._check(engine.lib().tsdbhip_batch_sizes(eng.ctx, C.byref(ns), C.byref(nr), C.byref(qb), C.byref(vb)))
    return nr.value


if __name__ == "__main__":
    main()
