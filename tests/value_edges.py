"""Helpers of the value-edge parity tests (test_value_edges_cpu.py, test_gpu_value_edges.py).

* cert_truth: the fact the engine's exactness certificate approximates, stated
  with exact rational arithmetic and not with the engine's formula;
* assert_bits / assert_rel: comparators without an absolute floor and with the sign of zero;
* builders of small stores whose values sit where a kernel can go wrong: at the certificate's
  threshold, past it (sums whose bits depend on the order), at the overflow threshold, signed
  zeros, NaN, +-Inf and a sweep of scales.

Every store is built per point in Python (synth.encode_rows): none holds more than ~150k points.
"""
from __future__ import annotations

import struct
from fractions import Fraction

import numpy as np

from opentsdb_amd import synth

T0 = 1356998400          # a multiple of 3600: hour rows start here
F32, F64, LONG = 1, 2, 0  # encode_rows kinds


# ---- the certificate's truth ------------------------------------------------------------------
def cert_truth(n: int, lsb: int, absmax: float) -> str:
    """n values, each a multiple of 2^lsb and no larger than absmax in magnitude.

    Every partial sum of them, in any order, is a multiple of 2^lsb bounded by n * absmax; a
    double holds such a number exactly when it is at most 2^53 * 2^lsb and below 2^1024.  Then
    every order of summation gives the same bits ("exact"); otherwise some order may round or
    overflow ("may_differ").  "must_take_fast" is the band a factor of two inside the engine's
    documented threshold 2^(52 + lsb): there the order-free kernels have no excuse to decline."""
    na = n * Fraction(absmax)
    two = Fraction(2)
    if na <= two ** (51 + lsb) and na < two ** 1023:
        return "must_take_fast"
    if na <= two ** (53 + lsb) and na < two ** 1024:
        return "exact"
    return "may_differ"


def lsb_of(x: float) -> int:
    """The largest e with x / 2^e an integer (x finite, non-zero), from the rational value."""
    num, den = Fraction(x).numerator, Fraction(x).denominator
    num = abs(num)
    return (num & -num).bit_length() - 1 - (den.bit_length() - 1)


def facts_of(values) -> tuple[int, float]:
    """(lsb, absmax) of a set of values, as the row index defines them."""
    fin = [float(v) for v in values if v == v and abs(v) != float("inf") and v != 0]
    lsb = min((lsb_of(v) for v in fin), default=None)
    return lsb, max((abs(float(v)) for v in values if v == v), default=0.0)


# ---- comparators ------------------------------------------------------------------------------
def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint64)


def assert_bits(got, want, ctx=""):
    """Group ids, timestamps, is_int and value bits (the sign of zero included) are equal; a NaN
    matches a NaN whatever its payload."""
    assert len(got) == len(want), f"{ctx}: {len(got)} groups vs {len(want)}"
    for (gg, t1, b1, i1), (wg, t2, b2, i2) in zip(got, want):
        assert gg == wg, f"{ctx}: group id {gg} != {wg}"
        assert len(t1) == len(t2), f"{ctx} g{gg}: {len(t1)} points vs {len(t2)}"
        np.testing.assert_array_equal(t1, t2, err_msg=f"{ctx} g{gg}: timestamps")
        np.testing.assert_array_equal(i1, i2, err_msg=f"{ctx} g{gg}: is_int")
        b1, b2 = _bits(b1), _bits(b2)
        fl = ~np.asarray(i2).astype(bool)
        n1 = np.zeros(len(b1), bool)
        n2 = np.zeros(len(b2), bool)
        n1[fl] = np.isnan(b1[fl].view(np.float64))
        n2[fl] = np.isnan(b2[fl].view(np.float64))
        np.testing.assert_array_equal(n1, n2, err_msg=f"{ctx} g{gg}: NaN positions")
        bad = np.flatnonzero((b1 != b2) & ~n1)
        if bad.size:
            k = int(bad[0])
            raise AssertionError(f"{ctx} g{gg}: {bad.size} values differ in bits, first at point {k} (ts {int(t1[k])}): "
                                 f"{b1[k]:#018x} ({b1[k:k + 1].view(np.float64)[0]!r}) != "
                                 f"{b2[k]:#018x} ({b2[k:k + 1].view(np.float64)[0]!r})")


def max_rel_err(got, want) -> float:
    """The largest |a - b| / |b| over the float values of two results of equal shape (b != 0)."""
    worst = 0.0
    for (_, _, b1, _), (_, _, b2, i2) in zip(got, want):
        fl = ~np.asarray(i2).astype(bool)
        a, b = _bits(b1)[fl].view(np.float64), _bits(b2)[fl].view(np.float64)
        ok = ~np.isnan(b) & (b != 0) & ~np.isinf(b)
        if ok.any():
            with np.errstate(over="ignore"):
                worst = max(worst, float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))))
    return worst


def assert_rel(got, want, tol, ctx=""):
    """A true relative comparison: |a - b| <= tol * |b|, and a == b where b is zero or infinite.
    Shape, timestamps, is_int, integer values and NaN positions as assert_bits."""
    assert len(got) == len(want), f"{ctx}: {len(got)} groups vs {len(want)}"
    for (gg, t1, b1, i1), (wg, t2, b2, i2) in zip(got, want):
        assert gg == wg, f"{ctx}: group id {gg} != {wg}"
        assert len(t1) == len(t2), f"{ctx} g{gg}: {len(t1)} points vs {len(t2)}"
        np.testing.assert_array_equal(t1, t2, err_msg=f"{ctx} g{gg}: timestamps")
        np.testing.assert_array_equal(i1, i2, err_msg=f"{ctx} g{gg}: is_int")
        b1, b2 = _bits(b1), _bits(b2)
        ints = np.asarray(i2).astype(bool)
        np.testing.assert_array_equal(b1[ints], b2[ints], err_msg=f"{ctx} g{gg}: integer values")
        a, b = b1[~ints].view(np.float64), b2[~ints].view(np.float64)
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=f"{ctx} g{gg}: NaN positions")
        ok = ~np.isnan(b)
        a, b = a[ok], b[ok]
        hard = (b == 0) | np.isinf(b)
        assert np.all(a[hard] == b[hard]), f"{ctx} g{gg}: a zero or infinite value is not matched"
        a, b = a[~hard], b[~hard]
        if a.size:
            with np.errstate(over="ignore"):
                err = np.abs(a - b) / np.abs(b)
            k = int(np.argmax(err))
            assert err[k] <= tol, f"{ctx} g{gg}: relative error {err[k]} > {tol} ({a[k]!r} vs {b[k]!r})"


# ---- sums in several orders (the CPU tests' evidence that a store is adversarial or not) -------
def seq_sum(v) -> float:
    s = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for x in np.asarray(v, np.float64):
            s = s + x
    return float(s)


def tree_sum(v) -> float:
    v = list(np.asarray(v, np.float64))
    with np.errstate(over="ignore", invalid="ignore"):
        while len(v) > 1:
            v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return float(v[0]) if v else 0.0


def bits_of(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def buckets_of(ts_ms, values, interval_ms):
    """The values of one series by bucket (ts - ts % interval), in time order."""
    out = {}
    for t, v in zip(ts_ms, values):
        out.setdefault(int(t) - int(t) % interval_ms, []).append(float(v))
    return out


# ---- stores -----------------------------------------------------------------------------------
class Store:
    """A batch with the values it was built from: series[i] = (ts_ms, values, kind)."""

    def __init__(self, series, gids):
        order = sorted(range(len(series)), key=lambda i: gids[i])   # (stable: batch order inside a group)
        self.series = [series[i] for i in order]
        self.gids = [gids[i] for i in order]
        rows = []
        for ts, v, kind in self.series:
            n = len(ts)
            if kind == LONG:
                rows.append(synth.encode_rows(ts, [int(x) for x in v], None, np.zeros(n, int), np.zeros(n, bool)))
            else:
                rows.append(synth.encode_rows(ts, None, np.asarray(v, np.float64), np.full(n, kind), np.zeros(n, bool)))
        self.batch = synth.from_series(rows, self.gids)

    @property
    def n_points(self):
        return sum(len(ts) for ts, _, _ in self.series)


def grid(n_rows: int, period_s: int, start=T0):
    """Timestamps (ms) of n_rows full hour rows at one point every period_s seconds."""
    return (start + np.arange(0, n_rows * 3600, period_s, dtype=np.int64)) * 1000


# the shapes that select each downsample path (tests/test_gpu_fast.py): (hour rows, period s)
SHAPES = {
    "one_row": (1, 10),      # 360 points in one row: k_short
    "rows": (3, 10),         # several one-chunk rows: k_rows
    "walker": (2, 1),        # rows of 3600 points (over one chunk): the k_fast row walker
    "short": (6, 600),       # 6 points an hour: rows k_seq_rows takes (under 64 datapoints a row)
}


def per_bucket(shape: str, interval_ms: int) -> int:
    return interval_ms // (SHAPES[shape][1] * 1000)


def odd_ints_store(e: int, shape: str, n_series=8, n_groups=2, seed=1, kind=F64) -> Store:
    """Odd integers just under 2^e (lsb 0, absmax < 2^e) as float cells, signs mixed."""
    rng = np.random.default_rng(seed)
    rows, period = SHAPES[shape]
    ts = grid(rows, period)
    series = []
    for s in range(n_series):
        v = (1 << e) - 1 - 2 * rng.integers(0, 1 << min(e - 2, 20), len(ts))
        v = v * rng.choice([-1, 1], len(ts))
        series.append((ts, v.astype(np.float64), kind))
    return Store(series, [s % n_groups for s in range(n_series)])


def big_odd_store(shape: str, n_series=8, n_groups=2, seed=2, e=48, base=None) -> Store:
    """Float64 cells base + odd (base 2^e): 60 of them add to ~1.9 * 2^53 at e = 48, past what a
    double holds exactly.  base = 7 * 2^48: five add to over 2^53 (an odd count: a rounding) while two still add exactly, so
    no row carries ROW_NOCERT and the kernel's own certificate has to decline."""
    rng = np.random.default_rng(seed)
    rows, period = SHAPES[shape]
    ts = grid(rows, period)
    base = (1 << e) if base is None else base
    series = [(ts, (base + 1 + 2 * rng.integers(0, 1 << 20, len(ts))).astype(np.float64), F64)
              for _ in range(n_series)]
    return Store(series, [s % n_groups for s in range(n_series)])


def f32_mixed_store(shape: str, m=30, k=30, n_series=8, n_groups=2, seed=3, big_every=2) -> Store:
    """Float32 cells odd * 2^-k with a 2^m every big_every-th point (big_every 0: one a row)."""
    rng = np.random.default_rng(seed)
    rows, period = SHAPES[shape]
    ts = grid(rows, period)
    per_row = 3600 // period
    series = []
    for _ in range(n_series):
        v = (2 * rng.integers(1 << 19, 1 << 23, len(ts)) + 1).astype(np.float64) * 2.0 ** -k
        if big_every:
            v[::big_every] = 2.0 ** m
        else:
            v[per_row // 2::per_row] = 2.0 ** m
        assert np.all(v.astype(np.float32).astype(np.float64) == v)
        series.append((ts, v, F32))
    return Store(series, [s % n_groups for s in range(n_series)])


def cross_row_store(n_rows=2, period=1, n_series=8, n_groups=2, seed=4, m=30, k=30) -> Store:
    """Hour rows that each certify alone -- row 1 only odd * 2^-k, the later rows only 2^m, as
    float32 -- so no row carries ROW_NOCERT; a bucket over the row boundary holds both."""
    rng = np.random.default_rng(seed)
    ts = grid(n_rows, period)
    per_row = 3600 // period
    series = []
    for _ in range(n_series):
        v = (2 * rng.integers(1 << 19, 1 << 23, len(ts)) + 1).astype(np.float64) * 2.0 ** -k
        v[per_row:] = 2.0 ** m
        series.append((ts, v, F32))
    return Store(series, [s % n_groups for s in range(n_series)])


HUGE = 2.0 ** 1023


def overflow_store(shape="one_row", partner=True) -> Store:
    """One series whose every 60-point run is [M, M, -M, -M] x 15, M = 2^1023 (Java's order
    reaches +Inf at the second value; an order-free sum can give 0 or +-M), and a partner of 1.0s."""
    rows, period = SHAPES[shape]
    ts = grid(rows, period)
    v = np.tile([HUGE, HUGE, -HUGE, -HUGE], len(ts) // 4)
    series, gids = [(ts, v, F64)], [0]
    if partner:
        series.append((ts, np.ones(len(ts)), F64))
        gids.append(0)
    return Store(series, gids)


# arrangements of +-M inside a bucket: Java's order reaches +-Inf in some and stays finite in
# others, while sums by lanes, pairs or trees cancel or overflow elsewhere
OVERFLOW_PATTERNS = {
    "MM-M-M": [1, 1, -1, -1], "M-M-MM": [1, -1, -1, 1], "-MMM-M": [-1, 1, 1, -1], "M-M": [1, -1],
    "MM-M-M-M-MMM": [1, 1, -1, -1, -1, -1, 1, 1], "M-MM-M-MM-MM": [1, -1, 1, -1, -1, 1, -1, 1],
}
OVERFLOW_STRIDES = (1, 2, 8, 15)   # every cell; every 2nd / 8th (one a lane of 8) / 15th, 0.0 between


def overflow_pattern_store(pattern: str, stride: int, shape="one_row") -> Store:
    """A series of +-2^1023 in the given arrangement at every stride-th cell (0.0 elsewhere: zeros
    leave lsb = 1023), and a partner of 1.0s in its group."""
    rows, period = SHAPES[shape]
    ts = grid(rows, period)
    v = np.zeros(len(ts))
    idx = np.arange(0, len(ts), stride)
    v[idx] = np.resize(np.array(OVERFLOW_PATTERNS[pattern], np.float64) * HUGE, len(idx))
    return Store([(ts, v, F64), (ts, np.ones(len(ts)), F64)], [0, 0])


def zeros_store(kind, first_sign: float, shape="one_row", n_series=4) -> Store:
    """Cells alternating +0.0 / -0.0, starting with first_sign (series s starts with the other
    sign when s is odd); one group a series."""
    rows, period = SHAPES[shape]
    ts = grid(rows, period)
    series = []
    for s in range(n_series):
        v = np.zeros(len(ts))
        sg = first_sign if s % 2 == 0 else -first_sign
        v[0::2] = np.copysign(0.0, sg)
        v[1::2] = np.copysign(0.0, -sg)
        series.append((ts, v, kind))
    return Store(series, list(range(n_series)))


def zero_groups_store(signs, kind=F64, shape="one_row") -> Store:
    """One group of len(signs) series, series i constant copysign(0, signs[i])."""
    rows, period = SHAPES[shape]
    ts = grid(rows, period)
    return Store([(ts, np.full(len(ts), np.copysign(0.0, s)), kind) for s in signs], [0] * len(signs))


def dyadic_base(n_series=6, n_groups=2, shape="one_row", seed=7):
    """(ts, [values]) multiples of 2^-10 below 2^10 (20 bits): 60 add exactly in any order, at any
    power-of-two scale that neither overflows nor runs below the smallest subnormal."""
    rng = np.random.default_rng(seed)
    rows, period = SHAPES[shape]
    ts = grid(rows, period)
    vals = [rng.integers(-(1 << 20) + 1, 1 << 20, len(ts)).astype(np.float64) * 2.0 ** -10 for _ in range(n_series)]
    return ts, vals, [s % n_groups for s in range(n_series)]


def scaled_store(s: int, kind=F64, **kw) -> Store:
    ts, vals, gids = dyadic_base(**kw)
    if kind == F32:   # 20-bit values: a float32 holds them down to its smallest normal; below, it rounds
        vals = [np.ldexp(v, s).astype(np.float32).astype(np.float64) for v in vals]
    else:
        vals = [np.ldexp(v, s) for v in vals]
    return Store([(ts, v, kind) for v in vals], gids)


def long_store(n_series=4, n_groups=2, shape="one_row", seed=8) -> Store:
    """8-byte integer cells +-(2^62 + odd)."""
    rng = np.random.default_rng(seed)
    rows, period = SHAPES[shape]
    ts = grid(rows, period)
    series = []
    for _ in range(n_series):
        v = [int(sg) * ((1 << 62) + 1 + 2 * int(o)) for sg, o in zip(rng.choice([-1, 1], len(ts)), rng.integers(0, 1 << 30, len(ts)))]
        series.append((ts, v, LONG))
    return Store(series, [s % n_groups for s in range(n_series)])


NAN = float("nan")
INF = float("inf")


def nan_store(case: str, kind=F32, shape="rows", n_series=6, n_groups=2, seed=9) -> Store:
    """Stores of values near 50 (certified) with NaN cells placed by `case` in every even series:
    bucket: one whole 60 s bucket; series: every cell; bucket_first / series_first: the first cell
    of one bucket / of the series; row: the whole middle hour row."""
    rng = np.random.default_rng(seed)
    rows, period = SHAPES[shape]
    ts = grid(rows, period)
    pb = 60 // period
    series = []
    for s in range(n_series):
        v = np.round(rng.normal(50, 5, len(ts)), 2).astype(np.float32).astype(np.float64)
        if s % 2 == 0:
            if case == "bucket":
                v[3 * pb:4 * pb] = NAN
            elif case == "series":
                v[:] = NAN
            elif case == "bucket_first":
                v[3 * pb] = NAN
            elif case == "series_first":
                v[0] = NAN
            elif case == "row":
                per_row = 3600 // period
                v[per_row:2 * per_row] = NAN
            else:
                raise ValueError(case)
        series.append((ts, v, kind))
    return Store(series, [s % n_groups for s in range(n_series)])


def inf_store(signs, kind=F64, shape="one_row", partner=True) -> Store:
    """Series 0 of 1.0s with the cells of its fourth 60 s bucket set to the infinities `signs`
    (one after the other from the bucket's start), and a finite partner series in its group."""
    rows, period = SHAPES[shape]
    ts = grid(rows, period)
    pb = 60 // period
    v = np.ones(len(ts))
    for i, sg in enumerate(signs):
        v[3 * pb + i] = sg * INF
    series, gids = [(ts, v, kind)], [0]
    if partner:
        series.append((ts, np.full(len(ts), 2.0), kind))
        gids.append(0)
    return Store(series, gids)


# ---- the datasets of the certificate tests: name -> (store factory, interval ms, (start s, end s)) ----
H = 3600
CERT_MAY_DIFFER = {
    # float64 2^48 + odd, 60 a bucket: n * A ~ 1.9 * 2^53
    "big_odd/one_row": (lambda: big_odd_store("one_row"), 600000, (T0, T0 + H - 1)),
    "big_odd/rows": (lambda: big_odd_store("rows"), 600000, (T0, T0 + 3 * H - 1)),
    "big_odd/walker": (lambda: big_odd_store("walker"), 60000, (T0, T0 + 2 * H - 1)),
    # K > 64 (1800 buckets of 4 s), 4 values of 2^52 + odd a bucket
    "big_odd52/walker/4s": (lambda: big_odd_store("walker", n_series=4, e=52), 4000, (T0, T0 + 2 * H - 1)),
    # float32 2^30 alternating with odd * 2^-30
    "f32_mixed/one_row": (lambda: f32_mixed_store("one_row"), 600000, (T0, T0 + H - 1)),
    "f32_mixed/rows": (lambda: f32_mixed_store("rows"), 600000, (T0, T0 + 3 * H - 1)),
    "f32_mixed/walker": (lambda: f32_mixed_store("walker"), 60000, (T0, T0 + 2 * H - 1)),
    # rows that certify alone, one bucket over both: 7 s buckets over the row boundary (K <= 64),
    # the same over two hours (K > 64), and one bucket of two hours
    "cross_row/7s": (lambda: cross_row_store(), 7000, (T0 + H - 200, T0 + H + 200)),
    "cross_row/7s/2h": (lambda: cross_row_store(), 7000, (T0, T0 + 2 * H - 1)),
    "cross_row/2h": (lambda: cross_row_store(), 2 * H * 1000, (T0, T0 + 2 * H - 1)),
    "cross_row/rows/2h": (lambda: cross_row_store(n_rows=3, period=10), 2 * H * 1000, (T0, T0 + 3 * H - 1)),
}
# one-chunk rows under 1m buckets over three hours (K = 180, 60 slots an hour: k_hwin's shape), six
# values a bucket; and rows of six points under 1h and 30m buckets (k_seq_rows' shape)
HWIN_Q = (60000, (T0, T0 + 3 * H - 1))
SHORT_WIN = (T0, T0 + 6 * H - 1)
CERT_MAY_DIFFER.update({
    "band/rows/1m": (lambda: big_odd_store("rows", base=7 << 48), *HWIN_Q),            # no ROW_NOCERT
    "big_odd52/rows/1m": (lambda: big_odd_store("rows", e=52), *HWIN_Q),               # ROW_NOCERT
    "f32_mixed/rows/1m": (lambda: f32_mixed_store("rows"), *HWIN_Q),
    "big_odd52/short/1h": (lambda: big_odd_store("short", e=52), 3600000, SHORT_WIN),
    "f32_mixed/short/1h": (lambda: f32_mixed_store("short"), 3600000, SHORT_WIN),
})
CERT_EXACT = {
    # (a): odd integers just under 2^e as float64, 60 a bucket; 45 is inside the engine's threshold
    # by a factor of two, 46 certifies, 47 does not (both still exact in truth), 48 is past it
    **{f"odd_ints/e{e}/{shape}": (lambda e=e, shape=shape: odd_ints_store(e, shape), iv, win)
       for e in (45, 46, 47)
       for shape, iv, win in (("one_row", 600000, (T0, T0 + H - 1)), ("walker", 60000, (T0, T0 + 2 * H - 1)))},
    # float32: odd * 2^-30 with one 2^m a row; m + 30 = 45 / 46 / 47
    **{f"f32_one_big/m{m}/{shape}": (lambda m=m, shape=shape: f32_mixed_store(shape, m=m, big_every=0), iv, win)
       for m in (15, 16, 17)
       for shape, iv, win in (("one_row", 600000, (T0, T0 + H - 1)), ("walker", 60000, (T0, T0 + 2 * H - 1)))},
}
CERT_EXACT.update({
    "odd_ints/e45/rows/1m": (lambda: odd_ints_store(45, "rows"), *HWIN_Q),
    "odd_ints/e50/rows/1m": (lambda: odd_ints_store(50, "rows"), *HWIN_Q),     # 6 * 2^50: in the band
    "f32_one_big/m15/rows/1m": (lambda: f32_mixed_store("rows", m=15, big_every=0), *HWIN_Q),
})
# (a) past the threshold: the truth no longer promises exactness (the kernels must decline); these
# stores happen to add exactly all the same -- which the CPU tests do not require
CERT_PAST = {
    "odd_ints/e48/one_row": (lambda: odd_ints_store(48, "one_row"), 600000, (T0, T0 + H - 1)),
    "odd_ints/e48/walker": (lambda: odd_ints_store(48, "walker"), 60000, (T0, T0 + 2 * H - 1)),
    "f32_one_big/m18/one_row": (lambda: f32_mixed_store("one_row", m=18, big_every=0), 600000, (T0, T0 + H - 1)),
}
# squareSum of odd integers under 2^e: lsb 0, squares under 2^(2e); 60 a bucket
SQ_E = {22: "must_take_fast", 23: "exact", 24: "may_differ"}


def series_truth(store: Store, interval_ms: int, square=False) -> str:
    """The weakest cert_truth over the store's series: n = the fullest bucket of the series."""
    rank = {"must_take_fast": 0, "exact": 1, "may_differ": 2}
    worst = "must_take_fast"
    for ts, v, _ in store.series:
        lsb, amax = facts_of(v)
        if lsb is None:
            continue
        n = max(len(x) for x in buckets_of(ts, v, interval_ms).values())
        t = cert_truth(n, 2 * lsb, amax * amax) if square else cert_truth(n, lsb, amax)
        if rank[t] > rank[worst]:
            worst = t
    return worst


# (g) the scale sweep: 2^s x the dyadic base
SCALES_F64 = [-1060, -140, -100, -40, 0, 40, 100, 960]
SCALES_F32 = [-140, -100, -40, 0, 40, 100]


def is_pure_scaling(base, scaled, s: int) -> bool:
    """Every float value of `scaled` is 2^s x the value of `base` at its place, bit for bit, and
    scaling it back returns the base value (nothing was lost on the way)."""
    if len(base) != len(scaled):
        return False
    for (g1, t1, b1, i1), (g2, t2, b2, i2) in zip(base, scaled):
        if g1 != g2 or not np.array_equal(t1, t2) or not np.array_equal(i1, i2):
            return False
        fl = ~np.asarray(i1).astype(bool)
        a, b = _bits(b1)[fl].view(np.float64), _bits(b2)[fl].view(np.float64)
        with np.errstate(over="ignore", under="ignore"):
            up = np.ldexp(a, s)
            back = np.ldexp(up, -s)
        ok = ~np.isnan(a)
        if not (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(up[ok].view(np.uint64), b[ok].view(np.uint64))
                and np.array_equal(back[ok], a[ok])):
            return False
    return True
