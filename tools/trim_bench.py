#!/usr/bin/env python3
"""tsdbhip_trim beside the only other way to drop an hour from a resident store, a tsdbhip_load of
the trimmed host batch -- the pack's stage time beside a device-to-device copy of the same bytes,
and the cost of a query step afterwards.  One JSON line a store.

Stores (device-synthesised, downloaded once, kept in page-locked arrays so that the load baseline
is a DMA upload): the tenths of tools/regroup_bench.py and tools/append_bench.py,
  c2   100k series x 3600 dp @1 s float32, 64 groups
  c3   1M series x 360 dp @10 s, integers / float32 alternating, 1000 groups
M holds two hour rows a series; the trim evicts the first hour, B is the trimmed batch.

  trim_nopack_ms /       host wall time of one call, alternating in one process: load(M) (not
  trim_pack_ms /         timed), trim(no pack); load(M), trim(pack); then load(B).  Median, min,
  load_ms                max of --repeats after --warmup.
  stages_ms              the trim's stages by hipEvents (option TRACE, read from stderr in a pass
                         of its own), without and with a pack: scan_gather, reindex, pack,
                         desc_download.  The pack stage is the two scans, the slack memsets, the
                         copy kernels and the offset rewrite.
  d2d_ms                 a hipMemcpyAsync device to device of the packed bytes (both blobs), by
                         events, in the same process; pack_over_d2d and pack_frac_of_copy_rate (read + write
                         bytes over the pack stage, as a fraction of 6.29 TB/s) follow from it.
  step_*_ms              host wall time of one sum:1m-avg tsdbhip_run (the C call alone):
                         --rounds alternations of 2 warm-ups + --steps timed calls in each state --
                         load(M) + regroup(hash) + trim(pack) against load(B with those ids);
                         load(M) + trim(no pack) against load(B); a second load(B) for the spread
                         between two fresh loads.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from append_bench import STORES, T0, interleave, pinned, stats   # noqa: E402

COPY_RATE = 6.29e12   # bytes/s, float4 copy on the device (read + write)


def traced(engine, fn, tag):
    """The stages option TRACE prints for the calls `fn` makes: {stage: [ms]}."""
    stages = {}
    with tempfile.TemporaryFile() as tf:
        saved = os.dup(2)
        try:
            sys.stderr.flush()
            os.dup2(tf.fileno(), 2)
            with engine.options(TRACE=1):
                fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tf.seek(0)
        for ln in tf.read().decode(errors="replace").splitlines():
            if ln.startswith(tag):
                for k, v in re.findall(r"(\w+) ([0-9.]+)", ln[len(tag):]):
                    stages.setdefault(k, []).append(float(v))
    return stages


def d2d_ms(nbytes, repeats):
    """hipMemcpyAsync device to device of nbytes, by hipEvents, through the HIP runtime the
    library has loaded."""
    import ctypes as C
    hip = None
    for name in ("libamdhip64.so.7", "libamdhip64.so"):   # (the soname resolves to the copy already loaded)
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            continue
    assert hip is not None, "the HIP runtime is not loadable by name"
    vp = C.c_void_p

    def ok(rc):
        assert rc == 0, f"hip error {rc}"

    src, dst, e0, e1 = vp(), vp(), vp(), vp()
    hip.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    hip.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    hip.hipEventDestroy.argtypes = [vp]
    hip.hipFree.argtypes = [vp]
    ok(hip.hipMalloc(C.byref(src), nbytes))
    ok(hip.hipMalloc(C.byref(dst), nbytes))
    ok(hip.hipEventCreate(C.byref(e0)))
    ok(hip.hipEventCreate(C.byref(e1)))
    out = []
    try:
        for i in range(repeats + 2):
            ok(hip.hipEventRecord(e0, None))
            ok(hip.hipMemcpyAsync(dst, src, nbytes, 3, None))   # hipMemcpyDeviceToDevice
            ok(hip.hipEventRecord(e1, None))
            ok(hip.hipEventSynchronize(e1))
            ms = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
            if i >= 2:
                out.append(ms.value)
    finally:
        for e in (e0, e1):
            hip.hipEventDestroy(e)
        for p in (src, dst):
            hip.hipFree(p)
    return out


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
    hash_ids = ((np.arange(n, dtype=np.int64) * 2654435761 >> 5) % sp["groups"]).astype(np.int32)
    M, B = pinned(engine, abi, m), pinned(engine, abi, b)
    Bh = abi.HostBatch(B.series_row_ptr, B.row_base_time, B.row_qual_off, B.row_val_off, B.qual, B.val,
                       engine.pinned_copy(hash_ids))
    del a, b, m
    cutoff = T0 + span
    q = abi.new_query(T0, T0 + 2 * span - 1, "sum", ds_function=abi.AGG["avg"], ds_interval_ms=60000)

    def same(r1, r2):
        assert len(r1) == len(r2) == sp["groups"]
        for (g1, t1, b1, _), (g2, t2, b2, _) in zip(r1, r2):
            assert g1 == g2 and np.array_equal(t1, t2)
            assert np.allclose(b1.view(np.float64), b2.view(np.float64), rtol=1e-9, atol=0)

    # ---- trim against load, alternating ----
    nop, pak, ld = [], [], []
    info = None
    for it in range(args.warmup + args.repeats):
        eng.load(M)
        eng.sync()
        t = time.perf_counter()
        i1 = eng.trim(cutoff, abi.TRIM_NO_PACK)
        d_np = (time.perf_counter() - t) * 1e3
        assert (i1.rows_evicted, i1.packed) == (n, 0)
        r1 = eng.run(q)
        eng.load(M)
        eng.sync()
        t = time.perf_counter()
        info = eng.trim(cutoff, 0)
        d_pk = (time.perf_counter() - t) * 1e3
        assert (info.rows_evicted, info.packed, info.qual_dead, info.val_dead) == (n, 1, 0, 0)
        r2 = eng.run(q)
        t = time.perf_counter()
        eng.load(B)
        d_ld = (time.perf_counter() - t) * 1e3
        r3 = eng.run(q)
        same(r1, r3)
        same(r2, r3)
        if it >= args.warmup:
            nop.append(d_np)
            pak.append(d_pk)
            ld.append(d_ld)
    live = int(info.qual_reclaimed + info.val_reclaimed)   # (two equal hours: the live bytes equal the reclaimed ones)

    # ---- the stages, by hipEvents ----
    def five(pack):
        for _ in range(5):
            eng.load(M)
            eng.trim(cutoff, pack)

    st_np = traced(engine, lambda: five(abi.TRIM_NO_PACK), "[trace trim]")
    st_pk = traced(engine, lambda: five(0), "[trace trim]")
    copy = d2d_ms(live, 5)
    med = statistics.median
    pack_ms = med(st_pk["pack"])
    # ---- the step afterwards ----
    step = {"trim_pack_regrouped": [], "load_regrouped": [], "trim_nopack": [], "load": [], "load2": []}
    for _ in range(args.rounds):
        for state in step:
            if state == "trim_pack_regrouped":
                eng.load(M)
                eng.regroup(hash_ids)
                eng.trim(cutoff, 0)
            elif state == "load_regrouped":
                eng.load(Bh)
            elif state == "trim_nopack":
                eng.load(M)
                eng.trim(cutoff, abi.TRIM_NO_PACK)
            else:
                eng.load(B)
            for i in range(2 + args.steps):
                eng.run(q)
                if i >= 2:
                    step[state].append(eng.last_call_ms)
    out = {
        "bench": "trim", "store": args.store, **sp, "rows_resident": 2 * n, "rows_evicted": n, "live_cell_bytes": live,
        "trim_nopack_ms": stats(nop), "trim_pack_ms": stats(pak), "load_ms": stats(ld),
        "nopack_over_load": round(med(nop) / med(ld), 5), "pack_over_load": round(med(pak) / med(ld), 5),
        "stages_nopack_ms": {k: stats(v) for k, v in st_np.items()},
        "stages_pack_ms": {k: stats(v) for k, v in st_pk.items()},
        "d2d_ms": stats(copy), "pack_over_d2d": round(pack_ms / med(copy), 4),
        "pack_frac_of_copy_rate": round(2 * live / (pack_ms * 1e-3) / COPY_RATE, 4),
        "d2d_frac_of_copy_rate": round(2 * live / (med(copy) * 1e-3) / COPY_RATE, 4),
        "qual_capacity": int(info.qual_capacity), "val_capacity": int(info.val_capacity),
        **{f"step_{k}_ms": stats(v) for k, v in step.items()},
        "step_pack_ratio": round(med(step["trim_pack_regrouped"]) / med(step["load_regrouped"]), 4),
        "step_nopack_ratio": round(med(step["trim_nopack"]) / med(step["load"]), 4),
        "step_load_spread": round(med(step["load2"]) / med(step["load"]), 4),
        "repeats": args.repeats, "warmup": args.warmup, "rounds": args.rounds, "steps": args.steps,
    }
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
