#!/usr/bin/env python3
"""tsdbhip_last over the config 3 one-hour store, and beside the only answer the engine had before
it: the last points of a `none`-aggregated raw query.  One JSON line a measurement.

The store is device-synthesised (Engine.synth): --series x 360 points @10 s in one hour row a
series, even series 1-2-byte integers in [0, 30000) (the copied route), odd series float32 (direct),
1000 groups.  Every series is anchored in that hour, back_scan 0, so every series answers.

  last_all     every series (a null selection), three ways in one process, alternating call by
               call so that they share the machine's state: as routed, under LAST_WALK=1 (every
               answer through k_last_walk), and a 1 % random selection (as routed).
  raw_none     on a --small store: tsdbhip_run of the `none` raw query, which decodes and returns
               every point, beside tsdbhip_last on the same store; the tool checks that the raw
               query's last points equal tsdbhip_last's answers.

  kernel_ms    info.kernel_ms: hipEvents around the call's two kernels
  wall_ms      host clock around the C call alone (outputs preallocated): uploads, kernels, the
               17 B a series back to pageable host memory, the synchronise
Median, min, max of --repeats calls after --warmup."""
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

T0 = 1356998400


def stats(x):
    return {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4)}


class Caller:
    """tsdbhip_last with every array allocated beforehand."""

    def __init__(self, engine, abi, eng, sel, n):
        self.L, self.eng, self.info = engine.lib(), eng, abi.LastInfo()
        self.sel = None if sel is None else np.ascontiguousarray(sel, np.int64)
        self.n = n if sel is None else len(self.sel)
        self.ts, self.bits, self.kind = np.zeros(self.n, np.int64), np.zeros(self.n, np.uint64), np.zeros(self.n, np.uint8)

    def __call__(self):
        t = time.perf_counter()
        rc = self.L.tsdbhip_last(self.eng.ctx, None if self.sel is None else self.sel.ctypes.data, self.n, T0 + 3599, None, 0,
                                 self.ts.ctypes.data, self.bits.ctypes.data, self.kind.ctypes.data, C.byref(self.info))
        wall = (time.perf_counter() - t) * 1e3
        assert rc == 0, rc
        return wall, self.info.kernel_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=10_000_000)
    ap.add_argument("--small", type=int, default=100_000, help="series of the store the raw query runs on (0: skip)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    args = ap.parse_args()
    from opentsdb_amd import abi, engine
    eng = engine.Engine(0)
    spec = dict(points=360, period_ms=10000, value_kind=2, groups=1000, int_mod=30000)

    def synth(n):
        eng.synth(n, T0, spec["points"], spec["period_ms"], spec["value_kind"], spec["groups"], spec["int_mod"], 0x5EED)

    # ---- every series, three ways ----
    n = args.series
    synth(n)
    rng = np.random.default_rng(1)
    calls = {"routed": (Caller(engine, abi, eng, None, n), None), "walk": (Caller(engine, abi, eng, None, n), 1),
             "select_1pct": (Caller(engine, abi, eng, rng.choice(n, max(1, n // 100), replace=False), n), None)}
    wall = {k: [] for k in calls}
    kern = {k: [] for k in calls}
    for it in range(args.warmup + args.repeats):
        for k, (call, walk) in calls.items():
            engine.set_option("LAST_WALK", walk)
            w, km = call()
            engine.set_option("LAST_WALK", None)
            if it >= args.warmup:
                wall[k].append(w)
                kern[k].append(km)
    routed, walked = calls["routed"][0], calls["walk"][0]
    for a, b in ((routed.ts, walked.ts), (routed.bits, walked.bits), (routed.kind, walked.kind)):
        assert np.array_equal(a, b)
    sel = calls["select_1pct"][0]
    assert np.array_equal(sel.ts, routed.ts[sel.sel]) and np.array_equal(sel.bits, routed.bits[sel.sel])
    assert (routed.kind != 0).all()
    for k, (call, walk) in calls.items():
        i = call.info
        print(json.dumps({"bench": "last_all", "how": k, "series": n, **spec, "n_sel": call.n, "found": int(i.found),
                          "direct": int(i.direct), "copied": int(i.copied), "walked": int(i.walked), "none": int(i.none),
                          "kernel_ms": stats(kern[k]), "wall_ms": stats(wall[k]),
                          "ns_per_series_kernel": round(statistics.median(kern[k]) * 1e6 / call.n, 3),
                          "repeats": args.repeats, "warmup": args.warmup}), flush=True)

    # ---- the parent commit's only answer: the raw `none` query's last points ----
    if args.small:
        m = args.small
        synth(m)
        q = abi.new_query(T0, T0 + 3599, "none")
        call = Caller(engine, abi, eng, None, m)
        raw, lw, lk = [], [], []
        res = None
        for it in range(args.warmup + args.repeats):
            res = eng.run(q)
            w, km = call()
            if it >= args.warmup:
                raw.append(eng.last_call_ms)
                lw.append(w)
                lk.append(km)
        # the raw query emits a span a series, keyed by its resident position; tsdbhip_last answers in batch order
        assert len(res) == m
        got = sorted((int(ts[-1]), int(np.asarray(bits).view(np.uint64)[-1])) for _, ts, bits, _ in res)
        assert got == sorted(zip(call.ts.tolist(), call.bits.tolist()))
        print(json.dumps({"bench": "raw_none", "series": m, **spec, "points_returned": int(sum(len(r[1]) for r in res)),
                          "raw_none_run_ms": stats(raw), "last_wall_ms": stats(lw), "last_kernel_ms": stats(lk),
                          "raw_over_last": round(statistics.median(raw) / statistics.median(lw), 1),
                          "repeats": args.repeats, "warmup": args.warmup}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
