"""Named stores for the percentile-downsampling edge tests (tests/test_pct_edges_cpu.py proves
they are what they claim, tests/test_gpu_pct_edges.py runs them on the device), a plain
restatement of one bucket's value, and a predictor of the route a query must take.

Every store is built with synth.encode_rows / synth.from_series from an exact, chosen number of
non-NaN values in every (series, bucket); the sizes sit on the thresholds of csrc/k_pct.hip:

* the sort size classes of bucket_value: <= CH (512) the register sort, 513 .. PCT_CAP (4096)
  sort_lds padded to 1024 / 2048 / 4096, above it the spill and the radix select;
* the rank edges of LEGACY pos = p (n + 1): the clamp to the maximum ends at n = 999 (p999),
  99 (p99), 19 (p95), 9 (p90), 3 (p75), 1 (p50);
* the extraction edges: a statistic within EXT_MAX = 24 of an end, up to n = 479 (p95), 239
  (p90), 95 (p75), 47 (p50), 48 (median);
* the 6-values-a-lane key kernel: longest certified row <= 384.

The restatement (bucket_value, restate) and the predictor (predict) are written from the rules
-- Aggregators.PercentileAgg / Median, and the conditions csrc/engine.cpp and k_pct_rows state in
their comments -- not read from the engine."""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np

from opentsdb_amd import abi, synth
from tests.rate_edges import scan_bounds, slots

T0 = 1356998400            # a multiple of 3 h
HOUR = 3600000
CH, PCT_CAP, EXT_MAX, V6_MAX = 512, 4096, 24, 384
INT32_MAX, INT32_MIN = (1 << 31) - 1, -(1 << 31)
FUNCS = ("p999", "p99", "p95", "p90", "p75", "p50", "median", "ep99r7")
QUANTILE = {"p999": 99.9, "p99": 99.0, "p95": 95.0, "p90": 90.0, "p75": 75.0, "p50": 50.0, "ep99r7": 99.0}
NEAR_END = ("p999", "p99", "p95", "p90", "ep99r7")        # k_pct_rows' extraction takes these; the rest are "mid"
SIZES = (1, 2, 3, 4, 9, 10, 19, 20, 24, 25, 47, 48, 49, 95, 96, 99, 100, 239, 240, 479, 480, 511, 512, 513, 999, 1000,
         1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 4160, 8191, 8192, 8193)
ROW_SIZES = tuple(sorted([n for n in SIZES if n <= CH] + [383, 384, 385]))
OPTION_SETS = ({}, {"PCT_V6": 0}, {"PCT_VONLY": 0}, {"PCT_KEYS": 0}, {"PCT_ROWS": 0})


# ---- one bucket, restated --------------------------------------------------------------------------
def total_order(x: float):
    """Double.compareTo on non-NaN values: -0.0 before 0.0."""
    return (x, math.copysign(1.0, x))


def ranks(fn: str, n: int):
    """(lo, hi, pos) of the sorted indices a function reads for n >= 1 values: median
    sorted[n // 2]; else commons-math3 LEGACY pos = p (n + 1), clamped to the ends."""
    if fn == "median":
        return n // 2, n // 2, 0.0
    if n == 1:
        return 0, 0, 0.0
    pos = (QUANTILE[fn] / 100.0) * (n + 1)
    if pos < 1:
        return 0, 0, pos
    if pos >= n:
        return n - 1, n - 1, pos
    return int(math.floor(pos)) - 1, int(math.floor(pos)), pos


def value_of_sorted(v, fn: str) -> float:
    n = len(v)
    if n == 0:
        return math.nan
    lo, hi, pos = ranks(fn, n)
    if lo == hi:
        return v[lo]
    lower, upper = v[lo], v[hi]
    dif = pos - math.floor(pos)
    return lower + dif * (upper - lower)


def bucket_value(values, fn: str) -> float:
    """Median.runDouble / PercentileAgg.runDouble over one bucket's values: NaNs dropped, sorted by
    the total order, sorted[n // 2] or the LEGACY estimate in doubles."""
    return value_of_sorted(sorted((float(x) for x in values if x == x), key=total_order), fn)


# ---- stores ------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    store: abi.HostBatch
    win: tuple          # (start s, end s) of the query
    I: int              # interval ms
    counts: dict        # (series, bucket start ms) -> intended non-NaN values (every non-empty bucket of the grid)
    classes: list       # per series: (qualifier width, value length) of every row, None = rows not pinned


def rows_of(ts, vals, kind, ms=False):
    """encode_rows of one series: kind 0 integers (vals are ints), 1 float32, 2 float64; or an array."""
    n = len(ts)
    kinds = np.full(n, kind) if np.isscalar(kind) else np.asarray(kind)
    lv = [int(v) if k == 0 else 0 for v, k in zip(vals, kinds)]
    fv = [0.0 if k == 0 else float(v) for v, k in zip(vals, kinds)]
    return synth.encode_rows(np.asarray(ts, np.int64), lv, fv, kinds, np.full(n, bool(ms)))


def decode(batch):
    """[series][row] = (base s, ts ms int64 [n], values float64 [n] as Span hands them out (an integer
    as (double) long), qualifier widths, value lengths, is-float flags), from the bytes."""
    qual, val = bytes(np.asarray(batch.qual, np.uint8)), bytes(np.asarray(batch.val, np.uint8))
    qo, vo = np.asarray(batch.row_qual_off).astype(np.int64), np.asarray(batch.row_val_off).astype(np.int64)
    srp = np.asarray(batch.series_row_ptr).astype(np.int64)
    out = []
    for s in range(len(srp) - 1):
        rows = []
        for r in range(int(srp[s]), int(srp[s + 1])):
            q, v = qual[qo[r]:qo[r + 1]], val[vo[r]:vo[r + 1]]
            base = int(batch.row_base_time[r])
            ts, xs, qws, vls, isf = [], [], [], [], []
            qi = vi = 0
            while qi < len(q):
                w = 4 if (q[qi] & 0xF0) == 0xF0 else 2
                off = ((int.from_bytes(q[qi:qi + 4], "big") & 0x0FFFFFC0) >> 6) if w == 4 else (int.from_bytes(q[qi:qi + 2], "big") >> 4) * 1000
                fl = q[qi + w - 1] & 0xF
                ln = (fl & 7) + 1
                raw = v[vi:vi + ln]
                if fl & 8:
                    x = float(np.frombuffer(raw, ">f4" if ln == 4 else ">f8")[0])
                else:
                    x = float(int.from_bytes(raw, "big", signed=True))
                ts.append(base * 1000 + off)
                xs.append(x)
                qws.append(w)
                vls.append(ln)
                isf.append(bool(fl & 8))
                qi += w
                vi += ln
            rows.append((base, np.asarray(ts, np.int64), np.asarray(xs, np.float64), qws, vls, isf))
        out.append(rows)
    return out


def grid_buckets(dec_series, win, I):
    """{bucket start ms: values in stored order} of one decoded series over the query's grid: the rows
    of the scan range, the buckets from the first boundary at or after the scan start."""
    q = abi.new_query(win[0], win[1], "none", ds_function=abi.AGG["p99"], ds_interval_ms=I)
    ss, se = scan_bounds(q)
    B0, K = slots(win, I)
    out = {}
    for base, ts, xs, *_ in dec_series:
        if not ss <= base < se:
            continue
        for t, x in zip(ts.tolist(), xs.tolist()):
            b = t - t % I
            if B0 <= b < B0 + K * I:
                out.setdefault(b, []).append(x)
    return out


def restate(batch, win, I, fns=FUNCS, dec=None):
    """{fn: [(group, ts, bits, is_int)]} as oracle.run_query gives it under the group-by aggregator
    `none`: every series with a row in the scan range is a group (numbered in batch order), its
    points the grid's buckets (the scan range, hour rows, bounds what is handed out, not the query's
    start and end), each bucket_value of the bucket's values."""
    dec = dec or decode(batch)
    out = {fn: [] for fn in fns}
    g = 0
    for rows in dec:
        gb = grid_buckets(rows, win, I)
        q = abi.new_query(win[0], win[1], "none", ds_function=abi.AGG["p99"], ds_interval_ms=I)
        ss, se = scan_bounds(q)
        if not any(ss <= r[0] < se for r in rows):
            continue
        keep = sorted(gb)
        srt = {b: sorted((x for x in gb[b] if x == x), key=total_order) for b in keep}
        for fn in fns:
            vals = np.array([value_of_sorted(srt[b], fn) for b in keep], np.float64)
            out[fn].append((g, np.asarray(keep, np.int64), vals.view(np.uint64).copy(), np.zeros(len(keep), np.uint8)))
        g += 1
    return out


def non_nan_counts(batch, win, I, dec=None):
    dec = dec or decode(batch)
    return {(s, b): sum(1 for x in xs if x == x) for s, rows in enumerate(dec) for b, xs in grid_buckets(rows, win, I).items()}


# ---- A: the size classes ------------------------------------------------------------------------------
A_I = 3 * HOUR
A_PATTERNS = ("distinct", "three", "equal", "clustered", "descending", "int64", "float32")
A_NAN_PATTERNS = ("distinct", "three", "float32")
A_NAN_EXTRA = {512: 8, 4096: 4, 4097: 103}     # raw 520 / 4100 / 4200: the raw count crosses, the kept one does not


def size_order():
    """SIZES with large and small buckets alternating (8193, 1, 8192, 2, ...), so that a small
    bucket follows a large one, and an empty bucket (None) between two full ones."""
    big, small = list(SIZES[::-1]), list(SIZES)
    out = []
    while len(out) < len(SIZES):
        out.append(big.pop(0))
        if len(out) < len(SIZES):
            out.append(small.pop(0))
    assert sorted(out) == sorted(SIZES)
    out.insert(5, None)
    return out


def pattern_values(pattern, n, rng, k):
    """(values, kind) of one bucket of n values."""
    if pattern == "distinct":            # full-mantissa doubles
        return rng.standard_normal(n) * 1e3, 2
    if pattern == "three":
        return rng.choice(np.array([-2.5, 0.125, 7e10]), n), 2
    if pattern == "equal":               # (the radix select's all-keys-equal exit)
        return np.full(n, 42.75 + k), 2
    if pattern == "clustered":           # shared leading digits: the radix select's prefix skip
        return 1e15 + rng.integers(0, 64, n).astype(np.float64), 2
    if pattern == "descending":
        return 1e4 - 0.37 * np.arange(n) + k, 2
    if pattern == "int64":
        return (1 << 40) + 3 * rng.integers(-1000, 1000, n), 0
    assert pattern == "float32"
    return rng.standard_normal(n).astype(np.float32).astype(np.float64), 1


@functools.lru_cache(maxsize=None)
def sizes_case(nans: bool) -> Case:
    """k_pct over every series (3 h does not divide the hour): one series a value pattern, every
    size of SIZES in every series (each series in its own rotation of size_order), points at 1 s
    from each bucket's start -- a bucket above 3600 values spans two hour rows.  nans: the same
    kept counts with NaNs interleaved (A_NAN_EXTRA at the thresholds, 1 .. 3 elsewhere), and a
    bucket of NaNs alone."""
    order = size_order() + (["nan"] if nans else [])
    nb = len(order)
    series, counts, classes = [], {}, []
    for s, pattern in enumerate(A_NAN_PATTERNS if nans else A_PATTERNS):
        rng = np.random.default_rng(1000 + s + (100 if nans else 0))
        rot = order[(5 * s) % nb:] + order[:(5 * s) % nb]
        ts_all, v_all, kind = [], [], 2
        for k, n in enumerate(rot):
            b = T0 * 1000 + k * A_I
            if n is None:
                continue
            if n == "nan":
                kept, extra = 0, 5
            else:
                kept, extra = n, (A_NAN_EXTRA.get(n, 1 + n % 3) if nans else 0)
            vals, kind = pattern_values(pattern, kept, rng, k)
            raw = np.full(kept + extra, np.nan)
            raw[np.sort(rng.choice(kept + extra, kept, replace=False))] = vals
            if kind == 0:
                raw = vals
            ts_all.append(b + 1000 * np.arange(kept + extra, dtype=np.int64))
            v_all.append(raw)
            counts[(s, b)] = kept
        series.append(rows_of(np.concatenate(ts_all), np.concatenate(v_all), kind))
        classes.append((2, {0: 8, 1: 4, 2: 8}[kind]))
    store = synth.from_series(series, [i % 2 for i in range(len(series))])
    return Case("sizes_nan" if nans else "sizes", store, (T0, T0 + nb * 10800 - 1), A_I, counts, classes)


# ---- B: rank edges inside k_pct_rows --------------------------------------------------------------------
B_CLASSES = [(qw, v) for qw in (2, 4) for v in ("i1", "i2", "i4", "f4", "i8", "f8")]
B_VL = {"i1": 1, "i2": 2, "i4": 4, "f4": 4, "i8": 8, "f8": 8}


def _class_values(v, n, rng, ties):
    if v == "i1":
        return rng.integers(-3, 4, n) if ties else rng.integers(-128, 128, n)
    if v == "i2":      # two bytes each: outside the int8 range
        x = rng.integers(128, 135, n) if ties else rng.integers(128, 32768, n)
        return np.where(rng.random(n) < 0.5, x, -x - 1)
    if v == "i4":      # four bytes each: outside the int16 range
        x = rng.integers(40000, 40006, n) if ties else rng.integers(32768, 1 << 31, n)
        return np.where(rng.random(n) < 0.5, x, -x - 1 + (x == INT32_MAX))     # (no INT32_MIN here)
    if v == "i8":
        x = rng.integers(1 << 40, (1 << 40) + 6, n) if ties else rng.integers(1 << 31, 1 << 52, n)
        return np.where(rng.random(n) < 0.5, x, -x - 1)
    if v == "f4":
        x = np.round(rng.normal(0, 20, n) * 2) / 2 if ties else rng.normal(0, 1e3, n)
        return x.astype(np.float32).astype(np.float64)
    assert v == "f8"
    return np.round(rng.normal(0, 20, n) * 2) / 2 if ties else rng.normal(0, 1e3, n)


def _offsets(qw, n, rng):
    if qw == 2:
        return np.sort(rng.choice(3600, n, replace=False)).astype(np.int64) * 1000
    return np.sort(rng.choice(HOUR, n, replace=False)).astype(np.int64)


def _rank_series(qw, v, sizes, rng, ties, nan_extra=0, rot=0, kinds=None):
    """One series: hour row h holds sizes[(h + rot) % len] non-NaN values (+ nan_extra NaNs where the row
    stays within 512).  Returns (ts, values, kind array, {bucket: kept})."""
    ts_all, v_all, k_all, counts = [], [], [], {}
    kind = 0 if v[0] == "i" else (1 if v == "f4" else 2)
    for h in range(len(sizes)):
        n = sizes[(h + rot) % len(sizes)]
        extra = min(nan_extra, CH - n)
        vals = _class_values(v, n, rng, ties).astype(np.float64 if kind else np.int64)
        raw = vals
        if extra:
            raw = np.full(n + extra, np.nan)
            raw[np.sort(rng.choice(n + extra, n, replace=False))] = vals
        b = T0 * 1000 + h * HOUR
        ts_all.append(b + _offsets(qw, n + extra, rng))
        v_all.append(raw)
        k_all.append(np.full(n + extra, kind) if kinds is None else kinds(n + extra, rng))
        counts[b] = n
    return np.concatenate(ts_all), np.concatenate(v_all), np.concatenate(k_all), counts


def _case_of(name, parts, win, I, classes, gids=None):
    series, counts = [], {}
    for s, (ts, vals, kinds, cnt) in enumerate(parts):
        series.append(rows_of(ts, vals, kinds, ms=False) if classes[s] is None or classes[s][0] == 2
                      else rows_of(ts, vals, kinds, ms=True))
        counts.update({(s, b): n for b, n in cnt.items()})
    store = synth.from_series(series, gids or [i % 2 for i in range(len(series))])
    return Case(name, store, win, I, counts, classes)


@functools.lru_cache(maxsize=None)
def rank_case(qw: int, v: str, longest: int = CH) -> Case:
    """One row class: series 0 distinct values, 1 ties, 2 ties in another rotation of the sizes, 3
    (float classes) NaNs added, which k_index certifies no longer; i4: series 3 holds INT32_MAX and
    INT32_MIN + 1 in every row, series 4 an INT32_MIN in every row (handed back by the key kernel).
    Rows hold ROW_SIZES values up to `longest`, one bucket each (1 h)."""
    sizes = tuple(n for n in ROW_SIZES if n <= longest)
    rng = np.random.default_rng(2000 + 10 * qw + B_CLASSES.index((qw, v)) + longest)
    parts = [_rank_series(qw, v, sizes, rng, False), _rank_series(qw, v, sizes, rng, True),
             _rank_series(qw, v, sizes, rng, True, rot=7)]
    if v == "f8":
        parts.append(_rank_series(qw, v, sizes, rng, True, nan_extra=3, rot=3))
    if v == "i4":
        for special in ((INT32_MAX, INT32_MIN + 1), (INT32_MIN, INT32_MIN)):
            ts, vals, kinds, cnt = _rank_series(qw, v, sizes, rng, True, rot=11)
            starts = np.flatnonzero(np.diff(np.concatenate([[-1], ts // HOUR])))
            for i, a in enumerate(starts):          # the row's first value, and (rows of >= 3) its third
                vals[a] = special[0]
                if a + 2 < len(vals) and (i + 1 == len(starts) or a + 2 < starts[i + 1]):
                    vals[a + 2] = special[1]
            parts.append((ts, vals, kinds, cnt))
    name = f"q{qw}{v}" + ("" if longest == CH else f"_{longest}")
    return _case_of(name, parts, (T0, T0 + len(sizes) * 3600 - 1), HOUR, [(qw, B_VL[v])] * len(parts))


@functools.lru_cache(maxsize=None)
def mixed4_case() -> Case:
    """4-byte values, not certified for the values-only kernel: series 0 and 1 rows that mix float32
    and int32 (the key kernel hands them back), 2 float32 with NaNs (it ranks them, counting the
    NaNs out), 3 int32."""
    rng = np.random.default_rng(2900)

    def mix(n, r):
        return np.where(r.random(n) < 0.5, 0, 1)
    parts = []
    for s in range(2):
        ts, vals, kinds, cnt = _rank_series(2, "f4", ROW_SIZES, rng, True, rot=5 * s, kinds=mix)
        ints = rng.integers(40000, 40006, len(vals))
        parts.append((ts, np.where(kinds == 0, ints, vals), kinds, cnt))
    parts.append(_rank_series(2, "f4", ROW_SIZES, rng, True, nan_extra=3, rot=2))
    parts.append(_rank_series(2, "i4", ROW_SIZES, rng, True, rot=9))
    return _case_of("mixed4", parts, (T0, T0 + len(ROW_SIZES) * 3600 - 1), HOUR, [(2, 4)] * 4)


B_CASES = {f"q{qw}{v}": functools.partial(rank_case, qw, v) for qw, v in B_CLASSES}
B_CASES["q2f4_384"] = functools.partial(rank_case, 2, "f4", 384)     # the ordinary certified float32 store: 6 values a lane
B_CASES["q2f4_385"] = functools.partial(rank_case, 2, "f4", 385)     # one value more: 8 values a lane
B_CASES["q4f4_384"] = functools.partial(rank_case, 4, "f4", 384)
B_CASES["mixed4"] = mixed4_case


# ---- C: sub-hour slots ----------------------------------------------------------------------------------
C_INTERVALS = (1000, 1125, 9375, 45000, 60000, 1800000)
C_ROW = 510          # datapoints a row: 170 boundaries, three offsets each


def slot_offsets(I):
    """The offsets k I - 1, k I, k I + 1 ms of every boundary k I of an hour row, with 0 and 3 599 999."""
    k = np.arange(0, HOUR // I + 1, dtype=np.int64)
    off = np.unique(np.concatenate([k * I - 1, k * I, k * I + 1]))
    return off[(off >= 0) & (off < HOUR)]


@functools.lru_cache(maxsize=None)
def slot_case(I: int, inside: bool = False) -> Case:
    """4-byte (millisecond) qualifiers with float32 values: the second hour row of series j holds the
    j-th 510 of slot_offsets(I) -- so the series together hold every boundary of the row, each within
    a row of one chunk --, the first hour row three points.  inside: the window starts half-way into
    the second row: the scan, and with it the grid, then starts at that row (slot 0 is the row's
    own base: a row in the scan range never lies before slot 0), and the first row is out of it."""
    off = slot_offsets(I)
    parts, base = [], (T0 + 3600) * 1000
    for j, a in enumerate(range(0, len(off), C_ROW)):
        o = off[a:a + C_ROW]
        ts = np.concatenate([T0 * 1000 + np.array([0, I - 1 if I > 1 else 1, HOUR - 1], np.int64), base + o])
        vals = (((np.arange(len(ts)) * 7919 + 13 * j) % 1009) * 0.25 - 100.0).astype(np.float32).astype(np.float64)
        cnt = {}
        for t in ts.tolist():
            cnt[t - t % I] = cnt.get(t - t % I, 0) + 1
        parts.append((ts, vals, np.full(len(ts), 1), cnt))
    win = (T0 + 3600 + 1800, T0 + 7199) if inside else (T0, T0 + 7199)
    if inside:
        parts = [(ts, v, k, {b: n for b, n in cnt.items() if b >= base}) for ts, v, k, cnt in parts]
    return _case_of(f"slots_{I}" + ("_inside" if inside else ""), parts, win, I, [(4, 4)] * len(parts))


# ---- D: the chain ---------------------------------------------------------------------------------------
D_HOURS = 3
CHAIN_10S = 10


@functools.lru_cache(maxsize=None)
def chain_case(n1s: int):
    """One batch, 1 h buckets: ten float32 series at 10 s (k_pct_rows launches, the values-only key
    kernel six values a lane); n1s series at 1 s (3600 a bucket: handed back, then the large-bucket
    pass's LDS sort); a series whose first row holds 4097 millisecond points (the radix select); a
    10 s series whose last row carries 20 more points at offsets 3600 .. 3790 s, the next hour's
    bucket (handed back after its first rows were written); a 10 s series whose second hour is two
    cells of one base time, which the load merges into one row (Span.addRow), so that the key kernel
    keeps the series.  Returns (case, series names)."""
    rng = np.random.default_rng(4000 + n1s)
    series, counts, classes, names = [], {}, [], []

    def f32(n):
        return (np.round(rng.normal(0, 50, n) * 4) / 4).astype(np.float32).astype(np.float64)

    def add(name, rows, cnt, cls):
        s = len(series)
        series.append(rows)
        counts.update({(s, b): n for b, n in cnt.items()})
        classes.append(cls)
        names.append(name)
    ts10 = T0 * 1000 + np.arange(D_HOURS * 360, dtype=np.int64) * 10000
    ts1 = T0 * 1000 + np.arange(D_HOURS * 3600, dtype=np.int64) * 1000
    hours = [T0 * 1000 + h * HOUR for h in range(D_HOURS)]
    for i in range(CHAIN_10S):
        add(f"f32_{i}", rows_of(ts10, f32(len(ts10)), 1), {b: 360 for b in hours}, (2, 4))
        if i == 2:
            for j in range(n1s):
                add(f"sec_{j}", rows_of(ts1, f32(len(ts1)), 1), {b: 3600 for b in hours}, (2, 4))
        if i == 4:
            tsm = T0 * 1000 + np.arange(4097, dtype=np.int64) * 877
            add("ms4097", rows_of(tsm, f32(4097), 1, ms=True), {hours[0]: 4097}, (4, 4))
        if i == 6:
            rows = rows_of(ts10, f32(len(ts10)), 1)
            base, q, v = rows[-1]
            q += b"".join((((3600 + 10 * k) << 4) | 0xB).to_bytes(2, "big") for k in range(20))
            v = v[:-1] + np.arange(20).astype(np.float32).astype(">f4").tobytes() + v[-1:]
            rows[-1] = (base, q, v)
            add("past_hour", rows, {**{b: 360 for b in hours}, T0 * 1000 + D_HOURS * HOUR: 20}, (2, 4))
        if i == 8:
            rows = rows_of(ts10, f32(len(ts10)), 1)
            base, q, v = rows[1]
            rows[1:2] = [(base, q[:360], v[:720] + v[-1:]), (base, q[360:], v[720:])]
            add("two_cells", rows, {b: 360 for b in hours}, (2, 4))
    store = synth.from_series(series, [i % 3 for i in range(len(series))])
    return Case(f"chain_{n1s}", store, (T0, T0 + (D_HOURS + 1) * 3600 - 1), HOUR, counts, classes), names


# ---- E: signed zeros and infinities -----------------------------------------------------------------------
# An infinity that reaches an output raises IllegalStateException (AggregationIterator, as for every
# downsampling function), so the stores come in two kinds: zeros_case, where every function's
# value is finite or NaN (infinities lie where no function reads, or where p999 interpolates
# between two of them: Inf - Inf), and inf_case, one bucket whose rank lands on an infinity for
# some functions -- there the outcome, the values or the exception, is what is compared.
E_SMALL, E_MID, E_BIG = (9, 20, 48, 100, 240, 512), (513, 1100), (4097,)
E_RANK_FUNCS = ("p999", "p99", "p95", "p90", "p75", "p50", "median")
E_ZERO_KINDS = ("nz|pz", "nz,pz", "inf,inf")
INF = math.inf


def _fill(n, r, split, rng):
    """n sorted values: -0.0 up to sorted index split - 1 and 0.0 from split (three of each where
    there is room), finite values of both signs around them."""
    nz, pz = min(3, split), min(3, n - split)
    lo = sorted((-(1.5 + rng.integers(0, 5, split - nz))).tolist())
    hi = sorted((2.5 + rng.integers(0, 5, n - split - pz)).tolist())
    return lo + [-0.0] * nz + [0.0] * pz + hi


def zero_bucket(n, r, kind, rng):
    """A multiset of n values, shuffled, whose sorted index r is -0.0 with 0.0 after it ("nz|pz") or
    0.0 with -0.0 before it ("nz,pz"); "inf,inf" (n >= 1000): the first, and +Inf from the lower
    index p999 reads to the top, so that p999 is Inf + dif (Inf - Inf).  Up to two -Inf below every
    index a function reads and up to two +Inf above them replace finite values."""
    r = min(r, n - 1)
    v = _fill(n, r, r if kind == "nz,pz" else r + 1, rng)
    assert len(v) == n
    lo_free = min(ranks(fn, n)[0] for fn in E_RANK_FUNCS)
    hi_free = n - 1 - max(ranks(fn, n)[1] for fn in E_RANK_FUNCS)
    for i in range(min(lo_free, 2)):
        v[i] = -INF if v[i] != 0 else v[i]
    for i in range(min(hi_free, 2)):
        v[n - 1 - i] = INF if v[n - 1 - i] != 0 else v[n - 1 - i]
    if kind == "inf,inf":
        lo999, hi999, _ = ranks("p999", n)
        assert hi999 == lo999 + 1 and lo999 > max(ranks(fn, n)[1] for fn in E_RANK_FUNCS[1:])
        v[lo999:] = [INF] * (n - lo999)
    out = np.array(sorted(v, key=total_order), np.float64)
    rng.shuffle(out)
    return out


@functools.lru_cache(maxsize=None)
def zeros_case(f64: bool) -> Case:
    """1 h buckets over the same multisets stored as float32 4-byte rows or as float64 8-byte rows:
    series 0 .. 5 rows of E_SMALL values at 1 s (the key kernel, or the extraction and the register
    sort), 6 and 7 rows of E_MID values at 1 s (sort_lds), 8 rows of 4097 values on millisecond
    qualifiers (the radix select).  Hour h of a series: the rank function h % 7 of E_RANK_FUNCS reads
    for that size, on the zero boundary kind h // 7 (1100 and 4097: "inf,inf" as well)."""
    rng = np.random.default_rng(5000 + int(f64))
    kind = 2 if f64 else 1
    parts, classes = [], []
    for n in E_SMALL + E_MID + E_BIG:
        kinds = E_ZERO_KINDS if n >= 1000 else E_ZERO_KINDS[:2]
        ts_all, v_all, cnt = [], [], {}
        for h in range(len(kinds) * len(E_RANK_FUNCS)):
            r = ranks(E_RANK_FUNCS[h % 7], n)[0]
            b = T0 * 1000 + h * HOUR
            ts_all.append(b + np.arange(n, dtype=np.int64) * (877 if n > 3600 else 1000))
            v_all.append(zero_bucket(n, r, kinds[h // 7], rng))
            cnt[b] = n
        parts.append((np.concatenate(ts_all), np.concatenate(v_all), np.full(sum(len(x) for x in v_all), kind), cnt))
        classes.append((4 if n > 3600 else 2, 8 if f64 else 4))
    return _case_of("zeros_f64" if f64 else "zeros_f32", parts, (T0, T0 + len(E_ZERO_KINDS) * 7 * 3600 - 1), HOUR, classes)


E_INF_KINDS = ("fin|inf", "inf,inf", "ninf,ninf")
E_INF_SIZES = (20, 240, 1100, 4097)
E_INF_FUNCS = ("p99", "p50")


@functools.lru_cache(maxsize=None)
def inf_case(f64: bool, n: int, kind: str, fn: str) -> Case:
    """Two series of one 1 h bucket each: series 0 holds n values whose sorted index r, the lower
    one `fn` reads, is a finite value with +Inf from r + 1 up ("fin|inf"), +Inf from r up
    ("inf,inf"), or -Inf up to r + 1 ("ninf,ninf"); series 1 twenty finite values.  A function
    whose rank lands on an infinity raises IllegalStateException; the others give their values."""
    rng = np.random.default_rng(5500 + n + int(f64))
    r = ranks(fn, n)[0]
    v = _fill(n, r, max(r - 2, 0), rng)
    if kind == "fin|inf":
        v[r:] = [1e30] + [INF] * (n - r - 1)
    elif kind == "inf,inf":
        v[r:] = [INF] * (n - r)
    else:
        m = min(r + 2, n)
        v[:m] = [-INF] * m
    vals = np.array(v, np.float64)
    rng.shuffle(vals)
    b = T0 * 1000
    k = 2 if f64 else 1
    parts = [(b + np.arange(n, dtype=np.int64) * (877 if n > 3600 else 1000), vals, np.full(n, k), {b: n}),
             (b + np.arange(20, dtype=np.int64) * 1000, np.arange(20) * 0.5 - 3.0, np.full(20, k), {b: 20})]
    classes = [(4 if n > 3600 else 2, 8 if f64 else 4), (2, 8 if f64 else 4)]
    return _case_of(f"inf_{'f64' if f64 else 'f32'}_{n}_{kind}_{fn}", parts, (T0, T0 + 3599), HOUR, classes)


# ---- the route a query must take ---------------------------------------------------------------------------
class Route(NamedTuple):
    launched: int       # k_pct_rows ran
    variant: int        # its KEYS code, -1 = none
    back: dict          # series -> why k_pct_rows hands it back
    big: set            # series with a bucket of more than 512 non-NaN values
    waves: int          # of the large-bucket pass
    cap_min: int        # big_cap is at least this

    def readout(self):
        return (self.launched, self.variant, len(self.back), len(self.big), self.waves)


def _far(fn, n):
    """The statistic of n values lies more than EXT_MAX from both ends."""
    lo, hi, _ = ranks(fn, n)
    return min(n - lo, hi + 1) > EXT_MAX


class Row(NamedTuple):
    """A row as the resident batch holds it, and what the load-time index says about it."""
    base: int
    ts: np.ndarray
    xs: np.ndarray
    isf: np.ndarray
    qw: int             # 2 or 4: every qualifier of that width, else 0
    vl: int             # the value length every datapoint has, else 0
    ndp: int
    allf: bool
    alli: bool
    nan: bool
    unsorted: bool      # an offset not after the one before it, or not after the series' earlier rows
    max_ms: int         # the latest offset from the base


def prepare(batch):
    """What predict derives from the bytes alone, for callers that predict many queries of one
    store: [series][row] Row.  Cells of one series with the same base time are one row: the load
    merges them as Span.addRow does (ordered by offset, the later cell's repeated timestamps
    dropped), so k_pct_rows' own check for a repeated base never fires on a loaded batch."""
    out = []
    for cells in decode(batch):
        rows, latest = [], -1
        i = 0
        while i < len(cells):
            base = cells[i][0]
            ts, xs, qws, vls, isf = (list(np.asarray(a).tolist()) for a in cells[i][1:])
            i += 1
            while i < len(cells) and cells[i][0] == base:
                seen = set(ts)
                add = [j for j, t in enumerate(cells[i][1].tolist()) if t not in seen]
                for dst, src in zip((ts, xs, qws, vls, isf), cells[i][1:]):
                    dst.extend(np.asarray(src)[add].tolist() if len(add) else [])
                order = sorted(range(len(ts)), key=lambda j: ts[j])      # (stable)
                ts, xs, qws, vls, isf = ([a[j] for j in order] for a in (ts, xs, qws, vls, isf))
                i += 1
            t = np.asarray(ts, np.int64)
            x = np.asarray(xs, np.float64)
            f = np.asarray(isf, bool)
            unsorted = bool(len(t) and ((np.diff(t) <= 0).any() or t[0] <= latest))
            if len(t):
                latest = max(latest, int(t.max()))
            rows.append(Row(base, t, x, f, qws[0] if len(set(qws)) == 1 else 0, vls[0] if len(set(vls)) == 1 and len(set(qws)) == 1 else 0,
                            len(t), bool(f.all()), bool((~f).all()), bool(np.isnan(x).any()), unsorted,
                            int((t - base * 1000).max()) if len(t) else -1))
        out.append(rows)
    return {"rows": out, "largest": {}}


def predict(batch, win, I, fn, opts=None, prep=None) -> Route:
    """What Engine.debug_pct() must show after fn-downsampling `batch` at interval I over `win`
    under the developer options `opts` ({name: 0} = off)."""
    opts = opts or {}
    on = lambda name: opts.get(name, 1) != 0      # noqa: E731
    prep = prep or prepare(batch)
    rows, largest = prep["rows"], prep["largest"]
    ns = len(rows)
    q = abi.new_query(win[0], win[1], "none", ds_function=abi.AGG[fn], ds_interval_ms=I)
    ss, se = scan_bounds(q)
    B0, K = slots(win, I)
    # the batch's k_pct_rows class: the (qualifier width, value length) with most datapoints in
    # sorted rows of one width and one length of at most 512 datapoints (ties: 2-byte qualifiers
    # first, then the shorter value); certified for the values-only kernel: every such row of the
    # class all float32 without NaN, or all int32
    cls, certified, longest = {}, {}, {}
    for f in (f for rr in rows for f in rr):
        if not f.unsorted and f.qw in (2, 4) and f.vl in (1, 2, 4, 8) and f.ndp <= CH:
            cls[(f.qw, f.vl)] = cls.get((f.qw, f.vl), 0) + f.ndp
            if f.vl == 4 and ((f.allf and not f.nan) or f.alli):
                certified[f.qw] = certified.get(f.qw, 0) + f.ndp
                longest[f.qw] = max(longest.get(f.qw, 0), f.ndp)
    best, qw, vl = 0, 0, 0
    for c in [(a, v) for a in (2, 4) for v in (1, 2, 4, 8)]:
        if cls.get(c, 0) > best:
            best, (qw, vl) = cls[c], c
    vonly = vl == 4 and best > 0 and certified.get(qw, 0) == best
    v6 = vonly and longest.get(qw, 0) <= V6_MAX
    near_end = fn in NEAR_END
    keys = vl == 4 and I == HOUR and on("PCT_KEYS")
    launched = bool((near_end or keys) and HOUR % I == 0 and B0 % I == 0 and best > 0 and on("PCT_ROWS") and ns > 0)
    variant, back = -1, {}
    if launched:
        vonly = keys and vonly and on("PCT_VONLY")
        v6 = vonly and v6 and on("PCT_V6")
        variant = 0 if not keys else (2 if not near_end else 1) + (4 if vonly else 0) + (8 if v6 else 0)
        for s in range(ns):
            why = None
            for f in rows[s]:          # the row descriptors first, a window of 64 rows at a time
                if not ss <= f.base < se:
                    continue
                if f.unsorted:
                    why = "an unsorted row"
                elif (f.qw, f.vl) != (qw, vl):
                    why = "a row of another class"
                elif f.ndp > CH:
                    why = "a row of more than 512 datapoints"
                elif f.base % 3600:
                    why = "a base off the hour"
                elif vonly and not ((f.allf and not f.nan) or f.alli):
                    why = "a row not certified"
                elif v6 and f.ndp > V6_MAX:
                    why = "a certified row of more than 384"
                if why:
                    break
            if why is None:        # then row by row, in order; the first that breaks a premise ends the series
                for f in rows[s]:
                    if not ss <= f.base < se or f.ndp == 0:
                        continue
                    if I == HOUR and not 0 <= (f.base * 1000 - B0) // I < K:
                        continue
                    if f.max_ms >= HOUR:
                        why = "an offset past the hour"
                    elif keys and ((~f.isf) & (f.xs == INT32_MIN)).any():
                        why = "an INT32_MIN value"
                    elif keys and not (f.allf or f.alli):
                        why = "a row of mixed kinds"
                    elif near_end:
                        b = f.ts - f.ts % I
                        kept = b[(b >= B0) & (b < B0 + K * I) & ~np.isnan(f.xs)]
                        if any(_far(fn, int(n)) for n in np.unique(kept, return_counts=True)[1]):
                            why = "a statistic more than 24 from both ends"
                    if why:
                        break
            if why:
                back[s] = why
    # k_pct, over the handed-back series or over all of them: a bucket of more than 512 kept values
    big = set()
    for s in (back if launched else range(ns)):
        if (s, win, I) not in largest:
            n = 0
            for f in rows[s]:
                if ss <= f.base < se:
                    b = f.ts - f.ts % I
                    kept = b[(b >= B0) & (b < B0 + K * I) & ~np.isnan(f.xs)]
                    for bb, c in zip(*np.unique(kept, return_counts=True)):
                        largest[(s, win, I, int(bb))] = largest.get((s, win, I, int(bb)), 0) + int(c)
                        n = max(n, largest[(s, win, I, int(bb))])
            largest[(s, win, I)] = n
        if largest[(s, win, I)] > CH:
            big.add(s)
    in_range = [sum(f.ndp for f in rows[s] if ss <= f.base < se) for s in range(ns)]
    cap_min = max([PCT_CAP + 1] + in_range) if big else 0
    waves = 0
    if big:
        waves = min(len(big), 4096, max(2, (2 << 30) // (cap_min * 8)))
        waves += waves & 1
    return Route(int(launched), variant, back, big, waves, cap_min)


# ---- the cases by name ----------------------------------------------------------------------------------------
A_CASES = {"sizes": functools.partial(sizes_case, False), "sizes_nan": functools.partial(sizes_case, True)}
C_CASES = {f"slots_{I}": functools.partial(slot_case, I) for I in C_INTERVALS}
C_CASES.update({f"slots_{I}_inside": functools.partial(slot_case, I, True) for I in (9375, 45000)})
D_N1S = (0, 1, 2, 3)
D_CASES = {f"chain_{n}": (lambda n=n: chain_case(n)[0]) for n in D_N1S}
E_CASES = {"zeros_f32": functools.partial(zeros_case, False), "zeros_f64": functools.partial(zeros_case, True)}
E_INF_CASES = {f"inf_{'f64' if f64 else 'f32'}_{n}_{kind}_{fn}": functools.partial(inf_case, f64, n, kind, fn)
               for f64 in (False, True) for n in E_INF_SIZES for kind in E_INF_KINDS for fn in E_INF_FUNCS}
CASES = {**A_CASES, **B_CASES, **C_CASES, **D_CASES, **E_CASES, **E_INF_CASES}


def query(case: Case, fn: str, agg: str = "none"):
    return abi.new_query(case.win[0], case.win[1], agg, ds_function=abi.AGG[fn], ds_interval_ms=case.I)
