#!/usr/bin/env python3
"""The sum:1m-avg step on one of tools/upsert_bench.py's stores (argument: c2 or c3) in six states
of one process, three alternations of 2 warm-ups + 5 timed calls: a fresh load of the merged
batch (twice), load + upsert of the 1 % delta, the same with APPEND_RESERVE=0, with a
tsdbhip_trim pack afterwards (the blobs re-laid in descriptor order, as a load lays them), and with
the upsert made twice (the second call does not grow).  One line a state: median, min, max, the
median of each alternation, and tsdbhip_debug_regular's lists."""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from append_bench import STORES, T0, pinned
from upsert_bench import subset
from opentsdb_amd import abi, engine
sp = dict(STORES[sys.argv[1]])
eng = engine.Engine(0)
span = 3600
eng.synth(sp["series"], T0 + span, sp["points"], sp["period_ms"], sp["value_kind"], sp["groups"], sp["int_mod"], 0xBEEF)
hour = eng.download(); n = hour.n_series
idx = np.arange(0, n, 100, dtype=np.int64)
D = pinned(engine, abi, subset(abi, hour, idx)); del hour
eng.synth(sp["series"], T0, 3 * sp["points"], sp["period_ms"], sp["value_kind"], sp["groups"], sp["int_mod"], 0x5EED)
M = pinned(engine, abi, eng.download())
z = np.zeros(len(idx), np.uint8)
eng.upsert(D, idx, z)
B = pinned(engine, abi, eng.download())
q = abi.new_query(T0, T0 + 3 * span - 1, "sum", ds_function=abi.AGG["avg"], ds_interval_ms=60000)
def st_load(): eng.load(B)
def st_upsert(): eng.load(M); eng.upsert(D, idx, z)
def st_upsert_r0():
    with engine.options(APPEND_RESERVE=0):
        eng.load(M); eng.upsert(D, idx, z)
def st_upsert_pack(): eng.load(M); eng.upsert(D, idx, z); eng.trim(0, 0)
def st_twice(): eng.load(M); eng.upsert(D, idx, z); eng.upsert(D, idx, z)
states = {"load": st_load, "upsert": st_upsert, "upsert_reserve0": st_upsert_r0, "upsert_pack": st_upsert_pack, "upsert_twice": st_twice, "load2": st_load}
out = {k: [] for k in states}
reg = {}
for rnd in range(3):
    for k, f in states.items():
        f()
        for i in range(7):
            eng.run(q)
            if i >= 2: out[k].append(eng.last_call_ms)
        fs, lists, launched = eng.debug_regular()
        reg[k] = (lists.tolist(), launched, int((fs[:, 1] != 0).sum()))
for k in out:
    print(k, "median %.4f min %.4f max %.4f" % (statistics.median(out[k]), min(out[k]), max(out[k])), "rounds", [round(statistics.median(out[k][i*5:(i+1)*5]), 4) for i in range(3)], "regular", reg[k])
eng.close()
