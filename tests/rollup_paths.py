"""Named stores for the rollup-generation route tests (tests/test_rollup_paths_cpu.py proves
they are what they claim, tests/test_gpu_rollup_paths.py runs them on the device).

Every store is tiny: 5-14 series over three hour rows.  T0 is itself an hour boundary, so the
series start five seconds before the next one, at START = T0 + 3595: a 5-second first row, a
full row of 7 chunks and a tail, and a partial last row of 700 s.  WIN0 = T0 + 3607 lies inside
the first lane of the second row's first chunk.

The streaming pass (k_rollup_fast) keeps its slots in LDS and runs only while
rollup_fast_lds(K) <= 32 KB, K <= 1170.  K is planned over whole hour rows (the scan range of
the window, not the window), so an hour of scan at interval I costs 3600 / I slots: the pass
cannot run under 1s, 2s or 3s cells whatever the window, under 5s only inside one hour row,
and from 7s on over two.  plan / window_k restate that plan, route_bounds the hand-backs the row classes force."""
from __future__ import annotations

import functools

import numpy as np

from opentsdb_amd import abi, synth

T0 = 1356998400
START = T0 + 3595          # first datapoint: 5 s before the second hour row
WIN0 = T0 + 3607           # inside the first lane of the second row's first chunk
SPAN_S = 5 + 3600 + 700    # seconds of data
END = START + SPAN_S       # one past the last whole second of data
H1, H2 = T0 + 3600, T0 + 7200
CH, DPL = 512, 8           # datapoints a chunk / a lane (kcommon.h)
K_FAST_MAX = 1170
FUNCS = (("sum", 0), ("count", 1), ("max", 2), ("min", 3))


def align16(x):
    return (x + 15) // 16 * 16


def rollup_fast_lds(K):
    """k_rollup.hip rollup_fast_wave_lds: three double arrays and one uint32 array of K slots."""
    return align16(K * 8) * 3 + align16(K * 4)


def plan(interval_s, start_s, end_s):
    """(B0 ms, K) of the Downsampler grid tsdbhip_rollup_run plans for a window: the query
    [start_s, end_s - 1] at the interval, first bucket at or after the scan start
    (TsdbQuery.getScanStartTimeSeconds / getScanEndTimeSeconds), slots up to the scan end."""
    from opentsdb_amd import engine
    I = interval_s * 1000
    q = abi.new_query(start_s, end_s - 1, "none", ds_function=abi.AGG["sum"], ds_interval_ms=I)
    ss, se = engine.scan_bounds(q)
    B0 = (ss * 1000 + I - 1) // I * I
    K = (se * 1000 - B0 + I - 1) // I if se * 1000 > B0 else 0
    return B0, K, ss, se


def window_k(interval_s, start_s, end_s):
    return plan(interval_s, start_s, end_s)[1]


def streams(interval_s, start_s, end_s):
    return rollup_fast_lds(window_k(interval_s, start_s, end_s)) <= 32 * 1024


def interval_seconds(interval):
    return int(interval[:-1]) * {"s": 1, "m": 60, "h": 3600, "d": 86400}[interval[-1]]


# ---- store access ---------------------------------------------------------------------------
def series_points(batch, s):
    """[(row base s, ts ms int64 [n] in stored order)] of series s, from the bytes."""
    out = []
    for r in range(int(batch.series_row_ptr[s]), int(batch.series_row_ptr[s + 1])):
        q = bytes(batch.qual[int(batch.row_qual_off[r]):int(batch.row_qual_off[r + 1])])
        base = int(batch.row_base_time[r])
        ts, i = [], 0
        while i < len(q):
            if (q[i] & 0xF0) == 0xF0:
                ts.append(base * 1000 + ((int.from_bytes(q[i:i + 4], "big") & 0x0FFFFFC0) >> 6))
                i += 4
            else:
                ts.append(base * 1000 + (int.from_bytes(q[i:i + 2], "big") >> 4) * 1000)
                i += 2
        out.append((base, np.asarray(ts, np.int64)))
    return out


def n_points(batch):
    return sum(len(ts) for s in range(len(batch.series_row_ptr) - 1) for _, ts in series_points(batch, s))


def runs(batch, s, interval_s, start_s, end_s):
    """Bucket runs of series s as the kernels see them: per row in the scan range and per
    512-datapoint chunk, (runs in the chunk, [runs in each 8-datapoint lane]).  A run is a
    stretch of consecutive datapoints of one slot; datapoints outside the grid are in none."""
    B0, K, ss, se = plan(interval_s, start_s, end_s)
    I = interval_s * 1000
    out = []
    for base, ts in series_points(batch, s):
        if not ss <= base < se:
            continue
        slot = np.where(ts >= B0, (ts - B0) // I, -1)
        slot[slot >= K] = -1
        for c0 in range(0, len(ts), CH):
            sl = slot[c0:c0 + CH]

            def count(a):
                a = a[a >= 0]
                return int(len(a) > 0) + int(np.count_nonzero(a[1:] != a[:-1]))
            out.append((count(sl), [count(sl[j:j + DPL]) for j in range(0, len(sl), DPL)]))
    return out


# ---- uniform classes ------------------------------------------------------------------------
def _npts(period_ms):
    return SPAN_S * 1000 // period_ms


@functools.lru_cache(maxsize=None)
def uniform(name):
    """One row class per store.  6 series in 3 groups (5 at 500 ms: under 45 000 datapoints)."""
    kind, period, n = {
        "q2f32": (0, 1000, 6), "q2f64": (3, 1000, 6), "q4f32": (0, 500, 5), "q4f64": (3, 500, 5),
        "vle8s": (1, 8000, 6), "vle7s": (1, 7000, 6),
        "fm1s": (4, 1000, 6), "fm500": (4, 500, 5),
    }[name]
    return synth.generate(n, START, _npts(period), period, value_kind=kind, n_groups=3, int_mod=30000)


CERTIFIED = ["q2f32", "q2f64", "q4f32", "q4f64", "vle8s", "vle7s"]
UNCERTIFIED = ["fm1s", "fm500"]
# (qualifier width, value length; 0 = vle) the index must find in every row
CLASS_OF = {"q2f32": (2, 4), "q2f64": (2, 8), "q4f32": (4, 4), "q4f64": (4, 8), "vle8s": (2, 0), "vle7s": (2, 0),
            "fm1s": (2, 8), "fm500": (4, 8)}


# ---- chain store ----------------------------------------------------------------------------
def _f32(seed, n):
    return synth.values(0x5EED, seed, np.arange(n, dtype=np.int64), 0, 0)[1]


def _rows(period_ms, seed, kind):
    """encode_rows of one regular series: kind 0 vle int16, 1 float32, 2 float64 of a float32, 4 full-mantissa float64."""
    n = _npts(period_ms)
    ts = START * 1000 + np.arange(n, dtype=np.int64) * period_ms
    ms = np.full(n, period_ms % 1000 != 0)
    k = np.arange(n, dtype=np.int64)
    if kind == 0:
        lv = synth.values(0x5EED, seed, k, 1, 30000)[1]
        return ts, lv, np.zeros(n), np.zeros(n, np.int64), ms
    fv = synth.values(0x5EED, seed, k, {1: 0, 2: 3, 4: 4}[kind], 0)[1].astype(np.float64)
    return ts, np.zeros(n, np.int64), fv, np.full(n, 1 if kind == 1 else 2), ms


CHAIN_SERIES = [
    # (name, group): batch order; groups interleaved, one series without a group in the middle
    ("f32_a", 2), ("vle_a", 0), ("late_nan", 1), ("q4f64_a", 3), ("f32_b", 0), ("fm", 2), ("vle_b", 1),
    ("nogroup", -1), ("late_int4", 3), ("f32_c", 1), ("q4f64_b", 0), ("vle_c", 2), ("late_ms", 0), ("f32_d", 3),
]
CHAIN_LATE = ("late_nan", "late_int4", "late_ms")


@functools.lru_cache(maxsize=None)
def chain():
    """Class A 2-byte/float32 (7 series at 1 s, 3 of them breaking a premise in their third row),
    class B vle int16 at 8 s, then what neither takes: 4-byte/float64 at 30.5 s and a
    full-mantissa series at 10 s (both with fewer datapoints than class B, so that the engine
    ranks them third), and a series without a group."""
    series = []
    for i, (name, _g) in enumerate(CHAIN_SERIES):
        if name.startswith("vle"):
            ts, lv, fv, kind, ms = _rows(8000, i, 0)
        elif name.startswith("q4f64"):
            ts, lv, fv, kind, ms = _rows(30500, i, 2)
        elif name == "fm":
            ts, lv, fv, kind, ms = _rows(10000, i, 4)
        else:
            ts, lv, fv, kind, ms = _rows(1000, i, 1)
        if name in CHAIN_LATE:
            j = int(np.searchsorted(ts, H2 * 1000)) + 300   # inside the third row's first chunk
            if name == "late_nan":
                fv[j] = np.nan
            elif name == "late_int4":
                kind[j], lv[j] = 0, 100000
            else:
                ms[j] = True
        series.append(synth.encode_rows(ts, lv, fv, kind, ms))
    return synth.from_series(series, [g for _, g in CHAIN_SERIES])


# ---- NaN store ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nans():
    """Float32 rows at 3 s.  Series 0 and 1 have no NaN (so the batch has a streaming class),
    the others 30 % NaN, series 2 nothing but NaN in its whole second row."""
    rng = np.random.default_rng(7)
    n = _npts(3000)
    ts = START * 1000 + np.arange(n, dtype=np.int64) * 3000
    series = []
    for s in range(8):
        fv = _f32(100 + s, n).astype(np.float64)
        if s >= 2:
            fv[rng.random(n) < 0.3] = np.nan
        if s == 2:
            fv[(ts >= H1 * 1000) & (ts < H2 * 1000)] = np.nan
        series.append(synth.encode_rows(ts, np.zeros(n, np.int64), fv, np.ones(n, np.int64), np.zeros(n, bool)))
    return synth.from_series(series, [s % 3 for s in range(8)])


# ---- stored-order stores --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stored_order(name):
    from tests.test_gpu_raw_unsorted import unsorted_batch
    if name == "swap_dup":
        return unsorted_batch(51, swap_p=0.25, dup_p=0.05)
    return unsorted_batch(52, swap_p=0.25, ms=True)


# ---- boundary store -------------------------------------------------------------------------
BOUNDARY_I = (7, 45)
BOUNDARY_WINDOW = (H1 + 7, H1 + 7190)   # (the scan of [H1, H1 + 2 h) at 7 s reaches a row either side)


def boundary_points(interval_s):
    """ts ms of the points one millisecond either side of, and on, every bucket boundary k * I
    inside [H1, H1 + 2 h), and their values (the position in the series, + 0.5)."""
    I = interval_s * 1000
    k = np.arange((H1 * 1000 + I - 1) // I, (H1 + 7200) * 1000 // I + 1, dtype=np.int64)
    ts = np.sort(np.concatenate([k * I - 1, k * I, k * I + 1]))
    ts = ts[(ts >= H1 * 1000) & (ts < (H1 + 7200) * 1000)]
    return ts, (np.arange(len(ts)) % 1000 + 0.5).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def boundary():
    """One class, 4-byte qualifiers with float32: 3 series on the 7 s boundaries, 3 on the 45 s ones."""
    series = []
    for I in BOUNDARY_I:
        ts, fv = boundary_points(I)
        for _ in range(3):
            series.append(synth.encode_rows(ts, np.zeros(len(ts), np.int64), fv, np.ones(len(ts), np.int64),
                                            np.ones(len(ts), bool)))
    return synth.from_series(series, [0, 1, 2, 0, 1, 2])


# ---- the GPU cases and the property each is named for -----------------------------------------
def a_window(interval):
    """Case a's window: from WIN0, min(1100 intervals, the data's end - 3 s) long."""
    return WIN0, min(WIN0 + 1100 * interval_seconds(interval), END - 3)


A_INTERVALS = [("1s", "1h"), ("2s", "1h"), ("3s", "1h"), ("5s", "1h"), ("7s", "1h"), ("13s", "1h"), ("45s", "1h"),
               ("90s", "1h"), ("1m", "1h"), ("5m", "1h"), ("1h", "1d")]
# windows inside the second hour row, where the streaming pass can still run under small cells
SHORT_WINDOW = (WIN0, H2)
# ... and 13s away from the hour's last 12 seconds: 276 cells of 13 s do not fill an hour row, and
# a bucket that starts in what is left is refused (RollupUtils.buildRollupQualifier), as it is
# for case a's own 13s window
A_SHORT = [("4s", "1h", SHORT_WINDOW), ("5s", "1h", SHORT_WINDOW), ("6s", "1h", SHORT_WINDOW),
           ("13s", "1h", (WIN0, H1 + 3580))]
# case c's windows: inside the second row (small K), and from the day's start over all three rows
C_WINDOWS = (SHORT_WINDOW, (T0, END))
C_INTERVALS = [("1s", "1h"), ("7s", "1h"), ("8s", "1h"), ("9s", "1h"), ("1m", "1h"), ("1h", "1d"), ("1d", "1n")]


# ---- the route a batch must take ------------------------------------------------------------
def _row_class(f, fl):
    """The streaming row class (qualifier width, value length; 0 = vle) a row counts for when the
    engine ranks the batch's classes, or None (engine.cpp finish_classes)."""
    from tests import index_ref as IR
    if f.err or fl & IR.ROW_UNSORTED:
        return None
    if f.allf and not f.nan and f.qw in (2, 4) and f.vl in (4, 8):
        return (f.qw, f.vl)
    if f.alli and f.vle2 and f.qw == 2 and f.ndp <= CH:
        return (2, 0)
    return None


def route_bounds(batch, interval_s, start_s, end_s):
    """(n, least series class A must hand back, least series the general kernel must reduce) of
    a streaming run: a series with a row of another class in the scan range cannot finish in a
    class.  Exact where every series that stays in its class also passes the certificate."""
    from tests import index_ref as IR
    _ndp, flags, _lsb, _amax, facts = IR.index_ref(batch)
    srp = np.asarray(batch.series_row_ptr).astype(int)
    gid = np.asarray(batch.group_id)
    _B0, _K, ss, se = plan(interval_s, start_s, end_s)
    dp = {}
    rows_of = []
    for s in range(len(srp) - 1):
        if gid[s] < 0:
            continue
        rr = [(int(batch.row_base_time[r]), _row_class(facts[r], int(flags[r])), facts[r]) for r in range(srp[s], srp[s + 1])]
        for _b, c, f in rr:
            if c:
                dp[c] = dp.get(c, 0) + f.ndp
        rows_of.append(rr)
    order = [(2, 4), (2, 8), (4, 4), (4, 8), (2, 0)]          # ties keep this order (a stable sort)
    rank = sorted((c for c in order if dp.get(c, 0) > 0), key=lambda c: -dp[c])
    A = rank[0] if rank else None
    B = rank[1] if len(rank) > 1 else None

    def stays(rr, c):
        return c is not None and all(rc == c and not (c[1] and f.negz) for b, rc, f in rr if ss <= b < se)
    n = len(rows_of)
    not_a = sum(1 for rr in rows_of if not stays(rr, A))
    neither = sum(1 for rr in rows_of if not stays(rr, A) and not stays(rr, B))
    return n, not_a, neither, A, B
