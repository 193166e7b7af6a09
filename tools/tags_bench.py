#!/usr/bin/env python3
"""tsdbhip_regroup_tags beside the way to the same state without it: tsdbhip_regroup with the ids
already computed -- which leaves out the host's id computation, so it is a lower bound for the
host path -- and the cost of a query step afterwards.  One JSON line a (store, query).

Stores (device-synthesised, as tools/regroup_bench.py):
  c2   a tenth of BASELINE config 2: 100k series x 3600 dp @1 s float32, 64 groups
  c3   a tenth of BASELINE config 3: 1M series x 360 dp @10 s, integers / float32 alternating,
       1000 groups
The synthetic tag table has four tags a series: dc = the store's group, host unique, rack of
cardinality 10, zone of cardinality 1000 (UIDs from 1, dense).
Queries: dc_star {dc=*}; dc3_host {dc=a|b|c, host=*}; rack_dc {rack=*, dc=literal}.

  tags_ms / ids_ms    host wall time of the C call alone, alternating order in one process: every
                      timed call starts from the all-ungrouped batch.  Median, min, max of
                      --repeats after --warmup.  diff_ms: the medians' difference, the cost of the
                      device part plus the ids' download.
  kernel_ms           info.kernel_ms of the timed calls; table_rate: table_bytes / kernel_ms over
                      the 6.29 TB/s float4-copy rate.
  python_group_ids_ms ResidentSpans.group_ids for the same query over the same tags: the Python
                      mirror's host path, not what a JVM would take.
  step_tags_ms /      one sum:1m-avg tsdbhip_run (the C call alone) after regroup_tags / after
  step_ids_ms         regroup: --rounds alternations of 2 warm-ups + --steps timed calls.
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

from tools.regroup_bench import STORES, T0, stats  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s, the float4 copy of DESIGN.md 7
DC, HOST, RACK, ZONE = 1, 2, 3, 4


class _Ids:
    def __init__(self, ids):
        self.ids = ids


class _Store:
    """The two UID dictionaries TsdbQuery's filter resolution reads."""

    def __init__(self, tagk, tagv):
        self.tagk, self.tagv = _Ids(tagk), _Ids(tagv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", choices=sorted(STORES), required=True)
    ap.add_argument("--series", type=int, default=0, help="override the store's series count (rehearsals)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--python-repeats", type=int, default=1)
    ap.add_argument("--sort", action="store_true", help="option TAGS_SORT=1: the sort route")
    args = ap.parse_args()
    from opentsdb_amd import abi, engine
    from opentsdb_amd.query import ResidentSpans, TsdbQuery
    sp = dict(STORES[args.store])
    if args.series:
        sp["series"] = args.series
    eng = engine.Engine(0)
    eng.synth(sp["series"], T0, sp["points"], sp["period_ms"], sp["value_kind"], sp["groups"], sp["int_mod"], 0x5EED)
    dc = np.asarray(eng.resident_groups(), np.int64)   # right after the synth: batch order
    n = len(dc)
    assert n == sp["series"] and dc.min() >= 0
    i = np.arange(n, dtype=np.int64)
    tagv = np.stack([dc + 1, i + 1, i % 10 + 1, (i * 2654435761 >> 9) % 1000 + 1], axis=1).astype(np.uint32)
    tagk = np.tile(np.asarray([DC, HOST, RACK, ZONE], np.uint32), n)
    ptr = np.arange(n + 1, dtype=np.int64) * 4
    t = time.perf_counter()
    eng.load_tags(ptr, tagk, tagv.reshape(-1))
    load_tags_ms = (time.perf_counter() - t) * 1e3
    if args.sort:
        engine.set_option("TAGS_SORT", 1)
    G = sp["groups"]
    lit = G // 2 + 1
    queries = {
        "dc_star": abi.HostTagQuery([(DC, abi.TF_ANY, [])], [DC]),
        "dc3_host": abi.HostTagQuery([(DC, abi.TF_IN, [1, lit, G]), (HOST, abi.TF_ANY, [])], [DC, HOST]),
        "rack_dc": abi.HostTagQuery([(RACK, abi.TF_ANY, []), (DC, abi.TF_IN, [lit])], [RACK]),
    }
    # the Python mirror's host path over the same tags: names are the UIDs' decimal strings
    names = {str(u): u for u in range(1, n + 2)}
    store = _Store({"dc": DC, "host": HOST, "rack": RACK, "zone": ZONE}, names)
    rs = ResidentSpans.__new__(ResidentSpans)
    rs.span_keys = [(0, tuple(zip((DC, HOST, RACK, ZONE), row))) for row in tagv.tolist()]
    rs.spans = [(sk, []) for sk in rs.span_keys]
    old_tags = {"dc_star": {"dc": "*"}, "dc3_host": {"dc": f"1|{lit}|{G}", "host": "*"}, "rack_dc": {"rack": "*", "dc": str(lit)}}
    end = T0 + sp["points"] * sp["period_ms"] // 1000
    step_q = abi.new_query(T0, end - 1, "sum", ds_function=abi.AGG["avg"], ds_interval_ms=60000)
    lib = engine.lib()
    none_ids = np.full(n, abi.GROUP_NONE, np.int32)
    out_ids = np.zeros(n, np.int32)
    info = abi.TagsInfo()
    flags = 0

    def call_tags(q):
        t = time.perf_counter()
        rc = lib.tsdbhip_regroup_tags(eng.ctx, C.byref(q.c), flags, out_ids.ctypes.data, C.byref(info))
        d = (time.perf_counter() - t) * 1e3
        engine._check(rc)
        return d

    def call_ids(ids):
        t = time.perf_counter()
        rc = lib.tsdbhip_regroup(eng.ctx, ids.ctypes.data, n)
        d = (time.perf_counter() - t) * 1e3
        engine._check(rc)
        return d

    for name, q in queries.items():
        tq = TsdbQuery(store)
        tq.tags = dict(old_tags[name])
        assert tq.tag_query() == q, name
        py = []
        for _ in range(args.python_repeats):
            t = time.perf_counter()
            py_ids, py_keys = rs.group_ids(tq)
            py.append((time.perf_counter() - t) * 1e3)
        ids_q = np.asarray(py_ids, np.int32)
        tg, rg, km = [], [], []
        for it in range(args.warmup + args.repeats):
            d = {}
            for which in (("tags", "ids") if it % 2 == 0 else ("ids", "tags")):
                engine._check(lib.tsdbhip_regroup(eng.ctx, none_ids.ctypes.data, n))
                d[which] = call_tags(q) if which == "tags" else call_ids(ids_q)
                if which == "tags":
                    assert np.array_equal(out_ids, ids_q), name
            if it >= args.warmup:
                tg.append(d["tags"])
                rg.append(d["ids"])
                km.append(info.kernel_ms)
        assert info.n_groups == len(py_keys)
        step = {"tags": [], "ids": []}
        for _ in range(args.rounds):
            for state in ("tags", "ids"):
                engine._check(lib.tsdbhip_regroup(eng.ctx, none_ids.ctypes.data, n))
                call_tags(q) if state == "tags" else call_ids(ids_q)
                for k in range(2 + args.steps):
                    eng.run(step_q)
                    if k >= 2:
                        step[state].append(eng.last_call_ms)
        k_med = statistics.median(km)
        print(json.dumps({
            "bench": "tags", "store": args.store, "query": name, "series": n, "groups_of_store": G,
            "route": info.route, "n_groups": info.n_groups, "visible": info.visible, "table_bytes": info.table_bytes,
            "load_tags_ms": round(load_tags_ms, 3),
            "tags_ms": stats(tg), "ids_ms": stats(rg), "diff_ms": round(statistics.median(tg) - statistics.median(rg), 4),
            "kernel_ms": stats(km), "table_rate": round(info.table_bytes / (k_med * 1e-3) / COPY_RATE, 5),
            "python_group_ids_ms": stats(py),
            "step_tags_ms": stats(step["tags"]), "step_ids_ms": stats(step["ids"]),
            "step_ratio": round(statistics.median(step["tags"]) / statistics.median(step["ids"]), 4),
            "repeats": args.repeats, "warmup": args.warmup, "rounds": args.rounds, "steps": args.steps,
            "sort_forced": bool(args.sort),
        }), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
