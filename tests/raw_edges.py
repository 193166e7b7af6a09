"""Helpers of the raw-path and group-by LERP edge tests (test_raw_edges_cpu.py,
test_gpu_raw_edges.py).

* ref_query: a plain Python restatement of the raw path -- AggregationIterator over the timestamp
  union (src/core/AggregationIterator.java:395-797), the aggregators' runLong / runDouble
  (src/core/Aggregators.java:231-851), the LEGACY / R_7 percentile estimate and RateSpan
  (src/core/RateSpan.java:112-180) -- for spans whose points are in time order.  Python ints
  wrapped to 64 bits stand for Java longs, Python floats for Java doubles; no numpy in the
  arithmetic.  It is a third leg beside the engine and the C oracle.
* builders of small stores whose points sit where the raw kernels can go wrong (the guards of the
  strip-wide long LERP, the limits of the corrected double division, products that wrap, NaN,
  infinities, signed zeros, subnormals, overflowing double LERPs, rate / counter edges and the
  strip geometry), and `sparse`, which removes whole buckets from a value_edges store so that
  the group-by of the downsampled path has to interpolate at the value edges.
"""
from __future__ import annotations

import math
import struct

import numpy as np

from opentsdb_amd import abi, synth
from tests import value_edges as V

T0, H = V.T0, V.H
LONG, F32, F64 = V.LONG, V.F32, V.F64
NAN, INF = V.NAN, V.INF
LONG_MAX, LONG_MIN = (1 << 63) - 1, -(1 << 63)
TIME_MASK = (1 << 63) - 1
M0 = T0 * 1000


def f32(x: float) -> float:
    """The double a float32 cell holding x decodes to."""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def dbits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---- stores -----------------------------------------------------------------------------------
class RStore:
    """A batch with the points it was built from: series[i] = [(ts_ms, kind, value)] in time
    order, kind per point (LONG / F32 / F64); a timestamp off the second takes a millisecond
    qualifier.  Series are ordered by group (stable), as value_edges.Store orders them."""

    def __init__(self, series, gids):
        order = sorted(range(len(series)), key=lambda i: gids[i])
        self.series = [[(int(t), k, (int(v) if k == LONG else f32(float(v)) if k == F32 else float(v)))
                        for t, k, v in series[i]] for i in order]
        self.gids = [gids[i] for i in order]
        rows = []
        for pts in self.series:
            assert all(a[0] < b[0] for a, b in zip(pts, pts[1:])), "points in time order"
            rows.append(synth.encode_rows([p[0] for p in pts], [p[2] if p[1] == LONG else 0 for p in pts],
                                          [0.0 if p[1] == LONG else p[2] for p in pts], [p[1] for p in pts],
                                          [p[0] % 1000 != 0 for p in pts]))
        self.batch = synth.from_series(rows, self.gids)

    @property
    def n_points(self):
        return sum(len(p) for p in self.series)


def span(ts, vals, kind):
    return [(t, kind, v) for t, v in zip(ts, vals)]


# ---- Java arithmetic --------------------------------------------------------------------------
def w64(x: int) -> int:
    return ((x + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


def jdiv(a: int, b: int) -> int:
    """Java long division: truncating, wrapping at Long.MIN_VALUE / -1."""
    q = abs(a) // abs(b)
    return w64(q if (a < 0) == (b < 0) else -q)


def jd2l(d: float) -> int:
    """(long) of a double (JLS 5.1.3)."""
    if d != d:
        return 0
    if d >= 9223372036854775807.0:
        return LONG_MAX
    if d <= -9223372036854775808.0:
        return LONG_MIN
    return int(d)


def jsqrt(x: float) -> float:
    return NAN if (x != x or x < 0) else math.sqrt(x)


class RefError(Exception):
    def __init__(self, java):
        super().__init__(java)
        self.java = java


# ---- Aggregators.java -------------------------------------------------------------------------
PCT = {"p999": 99.9, "p99": 99.0, "p95": 95.0, "p90": 90.0, "p75": 75.0, "p50": 50.0}


def _pct_of(name):
    """(quantile, estimation of runLong) of a percentile aggregator's name, or None."""
    if name in PCT:
        return PCT[name], "legacy"
    if name.startswith("ep") and name[-2:] in ("r3", "r7"):
        return PCT["p" + name[2:-2]], name[-2:]
    return None


def percentile(vals, quantile, est):
    """commons-math3 Percentile.evaluate: index() of LEGACY / R_3 / R_7 and the shared estimate()."""
    n = len(vals)
    if n == 0:
        return NAN
    if n == 1:
        return vals[0]
    work = sorted(vals, key=lambda x: (x, math.copysign(1.0, x)))   # Arrays.sort: -0.0 before 0.0
    p = quantile / 100.0
    if est == "r3":
        pos = 0.0 if p <= 0.5 / n else float(round(n * p))   # (rint: Python rounds half to even too)
    elif est == "r7":
        pos = 0.0 if p == 0.0 else float(n) if p == 1.0 else 1.0 + (n - 1) * p
    else:
        pos = 0.0 if p == 0.0 else float(n) if p == 1.0 else p * (n + 1)
    fpos = math.floor(pos)
    dif = pos - fpos
    if pos < 1:
        return work[0]
    if pos >= n:
        return work[n - 1]
    lower, upper = work[int(fpos) - 1], work[int(fpos)]
    return lower + dif * (upper - lower)


def run_long(name, v):
    """Aggregator.runLong over the values v (a non-empty list, in SpanGroup order)."""
    if name in ("sum", "pfsum", "zimsum"):
        r = v[0]
        for x in v[1:]:
            r = w64(r + x)
        return r
    if name == "squareSum":
        r = w64(v[0] * v[0])
        for x in v[1:]:
            r = w64(r + w64(x * x))
        return r
    if name in ("min", "mimmin"):
        m = v[0]
        for x in v[1:]:
            if x < m:
                m = x
        return m
    if name in ("max", "mimmax"):
        m = v[0]
        for x in v[1:]:
            if x > m:
                m = x
        return m
    if name == "avg":
        r = v[0]
        for x in v[1:]:
            r = w64(r + x)
        return jdiv(r, len(v))
    if name == "median":
        return sorted(v)[len(v) // 2]
    if name == "none":
        if len(v) > 1:
            raise RefError("IllegalDataException")
        return v[0]
    if name == "mult":
        r = v[0]
        for x in v[1:]:
            r = w64(r * x)
        return r
    if name == "dev":
        old = float(v[0])
        if len(v) == 1:
            return 0
        n, m2 = 2, 0.0
        for xl in v[1:]:
            x = float(xl)
            new = old + (x - old) / n
            m2 += (x - old) * (x - new)
            old = new
            n += 1
        return jd2l(jsqrt(m2 / (n - 1)))
    if name == "diff":
        return 0 if len(v) == 1 else w64(v[-1] - v[0])
    if name == "count":
        return len(v)
    if name == "first":
        return v[0]
    if name == "last":
        return v[-1]
    pq = _pct_of(name)
    if pq:
        return jd2l(percentile([float(x) for x in v], pq[0], pq[1]))
    raise ValueError(name)


def run_double(name, v):
    """Aggregator.runDouble over the values v (a non-empty list, in SpanGroup order)."""
    ok = [x for x in v if x == x]
    if name in ("sum", "pfsum", "zimsum", "avg", "squareSum"):
        r = 0.0
        for x in ok:
            r += x * x if name == "squareSum" else x
        if not ok:
            return NAN
        return r / len(ok) if name == "avg" else r
    if name in ("min", "mimmin"):
        m = INF if v[0] != v[0] else v[0]
        for x in v[1:]:
            if x == x and x < m:
                m = x
        return NAN if m == INF else m
    if name in ("max", "mimmax"):
        m = -INF if v[0] != v[0] else v[0]
        for x in v[1:]:
            if x == x and x > m:
                m = x
        return NAN if m == -INF else m
    if name == "median":
        if not ok:
            return NAN
        # Collections.sort of Doubles: Double.compareTo puts -0.0 before 0.0
        return sorted(ok, key=lambda x: (x, math.copysign(1.0, x)))[len(ok) // 2]
    if name == "none":
        if len(v) > 1:
            raise RefError("IllegalDataException")
        return v[0]
    if name == "mult":
        r = v[0]
        for x in v[1:]:
            r *= x
        return r
    if name in ("dev", "diff"):
        i = 0
        first = v[0]
        while first != first and i + 1 < len(v):
            i += 1
            first = v[i]
        if first != first:
            return NAN
        rest = v[i + 1:]
        if not rest:
            return 0.0
        if name == "diff":
            return rest[-1] - first
        old, n, m2 = first, 2, 0.0
        for x in rest:
            if x == x:
                new = old + (x - old) / n
                m2 += (x - old) * (x - new)
                old = new
                n += 1
        return 0.0 if n == 2 else jsqrt(m2 / (n - 1))
    if name == "count":
        return float(len(ok))
    if name == "first":
        return v[0]
    if name == "last":
        return v[-1]
    pq = _pct_of(name)
    if pq:
        return percentile(ok, pq[0], "legacy") if ok else NAN   # (runDouble ignores the estimation type)
    raise ValueError(name)


# ---- RateSpan.java ----------------------------------------------------------------------------
def rate_span(pts, counter, counter_max, reset_value, drop_resets):
    """The rates RateSpan hands out for the points [(ts, is_int, value)]: the first one against
    (0, 0L); a dropped reset still serves as the previous point of the next rate."""
    out = []
    prev = (0, True, 0)
    i = 0
    while i < len(pts):
        nxt = pts[i]
        i += 1
        secs = float(nxt[0] - prev[0]) / 1000.0
        both = prev[1] and nxt[1]
        diff = float(w64(nxt[2] - prev[2])) if both else float(nxt[2]) - float(prev[2])
        if counter and diff < 0:
            if drop_resets:
                prev = nxt
                continue
            if both:
                diff = float(w64(w64(counter_max - prev[2]) + nxt[2]))
            else:
                diff = float(counter_max) - float(prev[2]) + float(nxt[2])
            r = diff / secs
            out.append((nxt[0], False, 0.0 if (reset_value > 0 and r > float(reset_value)) else r))
        else:
            out.append((nxt[0], False, diff / secs))
        prev = nxt
    return out


# ---- AggregationIterator.java -------------------------------------------------------------------
def aggregate(views, start, end, agg, interp, rate):
    """[(ts, is_int, value)] of an AggregationIterator over the views [(ts, is_int, value)],
    restated slot by slot: timestamps / values / float flags of the current (i) and the next
    (size + i) point of every span."""
    size = len(views)
    ts, val, flt = [0] * (2 * size), [0] * (2 * size), [False] * (2 * size)
    nxt_idx = [0] * size

    def put_next(i):
        v = views[i]
        if nxt_idx[i] < len(v):
            t, is_int, x = v[nxt_idx[i]]
            nxt_idx[i] += 1
            ts[size + i], val[size + i], flt[size + i] = t, x, not is_int
        else:
            ts[size + i], flt[size + i] = TIME_MASK, False   # endReached

    def move(i):
        ts[i], val[i], flt[i] = ts[size + i], val[size + i], flt[size + i]
        put_next(i)

    for i in range(size):
        views[i] = [p for p in views[i] if p[0] >= start]   # seek + "advance to the start time"
        put_next(i)
        if rate and ts[size + i] != TIME_MASK:
            if nxt_idx[i] < len(views[i]):
                move(i)
            else:
                ts[size + i], flt[size + i] = TIME_MASK, False
    out = []
    current = 0
    while any(ts[size + i] <= end for i in range(size)):
        for i in range(current, size):
            if ts[size + i] == TIME_MASK:
                ts[i], flt[i] = 0, False
        current, min_ts, multiple = -1, LONG_MAX, False
        for i in range(size):
            t = ts[size + i]
            if t <= end:
                if t < min_ts:
                    min_ts, current, multiple = t, i, False
                elif t == min_ts:
                    multiple = True
        move(current)
        if multiple:
            for i in range(current + 1, size):
                if ts[size + i] == min_ts:
                    move(i)
        x = ts[current]
        is_int = not rate and not any(flt)
        vals = []
        for pos in range(size):
            if ts[pos] == 0:
                continue
            if is_int:
                y0 = val[pos]
                if current == pos or x == ts[pos]:
                    vals.append(y0)
                    continue
                y1, x0, x1 = val[size + pos], ts[pos], ts[size + pos]
                if x == x1:
                    vals.append(y1)
                elif interp == abi.INTERP_LERP:
                    vals.append(w64(y0 + jdiv(w64((x - x0) * w64(y1 - y0)), x1 - x0)))
                else:
                    vals.append({abi.INTERP_ZIM: 0, abi.INTERP_MAX: LONG_MAX, abi.INTERP_MIN: LONG_MIN,
                                 abi.INTERP_PREV: y0}[interp])
            else:
                y0 = float(val[pos])
                if current == pos or rate or x == ts[pos]:
                    vals.append(y0)
                    continue
                y1, x0, x1 = float(val[size + pos]), ts[pos], ts[size + pos]
                if x == x1:
                    vals.append(y1)
                elif interp == abi.INTERP_LERP:
                    vals.append(y0 + float(x - x0) * (y1 - y0) / float(x1 - x0))
                else:
                    vals.append({abi.INTERP_ZIM: 0.0, abi.INTERP_MAX: 1.7976931348623157e308,
                                 abi.INTERP_MIN: 4.9e-324, abi.INTERP_PREV: y0}[interp])
        if is_int:
            out.append((x, True, run_long(agg, vals)))
        else:
            r = run_double(agg, vals)
            if r in (INF, -INF):
                raise RefError("IllegalStateException")   # "Got Infinity" (:640-643)
            out.append((x, False, r))
    return out


def scan_bounds(q):
    """TsdbQuery's scan range in seconds of a query without a downsampler: whole hour rows."""
    s, e = q.start_time, q.end_time
    return s - s % 3600, e + (3600 - e % 3600)


def ref_query(store: RStore, q):
    """The query on the Python reference: [(group id, ts, bits, is_int)] as oracle.run_query
    returns it, or RefError with the Java exception's name."""
    assert q.ds_function < 0 or q.ds_interval_ms == 0, "the raw path only"
    name = abi.AGGREGATOR_NAMES[q.aggregator]
    ss, se = scan_bounds(q)
    spans = []
    for pts, gid in zip(store.series, store.gids):
        kept = [(t, k == LONG, v) for t, k, v in pts if ss <= (t // 1000 - t // 1000 % 3600) < se]
        if kept:
            spans.append((gid, kept))
    if name == "none":
        groups = [(i, [s[1]]) for i, s in enumerate(spans)]
    else:
        groups = [(g, [s[1] for s in spans if s[0] == g]) for g in sorted({s[0] for s in spans})]
    out = []
    for gid, views in groups:
        if q.rate:
            views = [rate_span(v, bool(q.rate_counter), q.rate_counter_max, q.rate_reset_value,
                               bool(q.rate_drop_resets)) for v in views]
        pts = aggregate(list(views), ss * 1000, se * 1000, name, abi.interpolation_of(q.aggregator), bool(q.rate))
        out.append((gid, np.array([p[0] for p in pts], np.int64),
                    np.array([(p[2] & ((1 << 64) - 1)) if p[1] else dbits(p[2]) for p in pts], np.uint64),
                    np.array([1 if p[1] else 0 for p in pts], np.uint8)))
    return out


def ref_outcome(store, q):
    try:
        return ref_query(store, q), None
    except RefError as e:
        return None, e.java


def union_of(store: RStore, gid: int, win):
    """The sorted timestamp union of a group inside the scan range of the window (s, e)."""
    ss, se = win[0] - win[0] % 3600, win[1] + (3600 - win[1] % 3600)
    return sorted({t for pts, g in zip(store.series, store.gids) if g == gid
                   for t, _, _ in pts if ss * 1000 <= t < se * 1000})


# ---- A.1 the guards of the strip-wide long LERP ---------------------------------------------------
WINDOW_DENS = (3, 1000, 4096, 3600000)
STRIP = 512          # union points a k_raw_eval wave takes
WIN_X0 = M0 + 2000   # every window starts here: 511 clock points lie before it


def window_dys(den: int):
    """dy of both signs at the guards of lerpw_init (rounded product < 2^50, |dy| < 2^51) and
    next to them, exact multiples of den (remainder 0 and -0) and their neighbours."""
    mags = []
    for top in (50, 51):
        f = (1 << top) // den
        mags += [f - 1, f, f + 1]
    mags += [(1 << 51) - 1, 1 << 51, (1 << 51) + 1]
    for k in (1, 7, 12345):
        mags += [k * den, k * den - 1, k * den + 1]
    k = max(1, ((1 << 50) // den - 3) // den)   # the largest multiple of den inside the guard
    mags += [k * den, k * den - 1, k * den + 1]
    out = []
    for m in mags:
        if m > 0 and m not in out:
            out.append(m)
    return [s * m for m in out for s in (1, -1)]


def window_eval_points(den: int):
    return sorted({1, den // 2, den - 1} - {0, den})


def window_clock(den: int):
    """Timestamps of the partner: 511 points before the window (its first point gets rank 511,
    the last of strip 0), then points strictly inside it -- x0 + 1, the midpoint, x1 - 1 and up to
    700 more: with den >= 1000 strip 1 lies wholly inside the window (m == 0: the strip-wide
    path), strips 0 and 2 hold its ends (m > 0: the general path) -- and five points after it."""
    x0 = WIN_X0
    before = [x0 - (STRIP - 1) + i for i in range(STRIP - 1)]
    inner = set(window_eval_points(den))
    n_in = min(den - 1, 700)
    inner |= {1 + (i * (den - 2)) // max(n_in - 1, 1) for i in range(n_in)} if den > 2 else set()
    after = [x0 + den + 1000 * (i + 1) for i in range(5)]
    return before + [x0 + d for d in sorted(inner)] + after


def window_store(den: int, y0=-7) -> RStore:
    """One group a dy: the window span (x0, y0), (x1, y0 + dy) and the partner clock of small
    integers (so that the group stays in long arithmetic)."""
    clock = window_clock(den)
    series, gids = [], []
    for g, dy in enumerate(window_dys(den)):
        series.append(span([WIN_X0, WIN_X0 + den], [y0, y0 + dy], LONG))
        series.append(span(clock, [(i * 37) % 101 - 50 for i in range(len(clock))], LONG))
        gids += [g, g]
    return RStore(series, gids)


def lerpw_branch(dx, den, dy):
    """Which correction lerpw_eval applies at x - x0 = dx ("none", "r>=den", "r<0", "r>0",
    "r<=-den"), with the arithmetic of tests/test_lerp_window_math.lerpw."""
    nd = float(dx) * float(dy)
    q = float(math.trunc(nd * (1.0 / float(den))))
    r = int(nd) - int(q) * den
    if dy >= 0:
        return "r>=den" if r >= den else "r<0" if r < 0 else "none"
    return "r>0" if r > 0 else "r<=-den" if r <= -den else "none"


# ---- A.3 jdiv_pos: |product| at 2^53 and products that wrap ----------------------------------------
# (dx, dy) with dx * dy = 2^53 - 1, 2^53, 2^53 + 1, and a few around them
JDIV_PRODUCTS = [(6361, 69431 * 20394401), (1024, 1 << 43), (321, 28059810762433), (3, 107 * 28059810762433),
                 (1023, 1 << 43), (1025, 1 << 43), (4095, (1 << 41) + 1)]
JDIV_WRAPS = [  # (y0, y1): y1 - y0 wraps or nearly does; times dx = 3, 5, 4001 the product wraps once, twice, often
    (LONG_MAX - 5, -3), (LONG_MIN + 7, 11), (LONG_MAX - 5, LONG_MIN + 9), (LONG_MIN + 7, LONG_MAX - 1),
    (LONG_MAX, 0), (LONG_MIN, -1), (LONG_MIN, LONG_MAX), ((1 << 62) + 1, -(1 << 62) - 3),
    ((1 << 61) + 3, -(1 << 61) - 1), (LONG_MAX - 5, (1 << 62) + 1), (LONG_MIN + 7, -(1 << 62) - 1)]
JDIV_DEN = 7000


def jdiv_store() -> RStore:
    series, gids = [], []
    x0 = M0 + 5000
    g = 0
    for dx, dy in JDIV_PRODUCTS:
        assert dx < JDIV_DEN
        for sg in (1, -1):
            series.append(span([x0, x0 + JDIV_DEN], [11, 11 + sg * dy], LONG))
            series.append(span([x0 - 1000, x0 + dx, x0 + JDIV_DEN - 1, x0 + JDIV_DEN + 1000], [1, -2, 3, -4], LONG))
            gids += [g, g]
            g += 1
    for y0, y1 in JDIV_WRAPS:
        series.append(span([x0, x0 + JDIV_DEN], [y0, y1], LONG))
        series.append(span([x0 - 1000, x0 + 3, x0 + 5, x0 + 4001, x0 + JDIV_DEN + 1000], [1, -2, 3, -4, 5], LONG))
        gids += [g, g]
        g += 1
    return RStore(series, gids)


# ---- A.4 double LERP values ------------------------------------------------------------------------
S = 1000


def _lerp_group(ends, kind, partner_vals=(1.5, -2.25, 3.0, 0.5, 7.0), pk=None, n=5):
    """A span of the values `ends` at 0 s, 100 s, 200 s ... and a partner with points between
    them (10 s, 50 s, 99.999 s after every end) and before / after the span."""
    t = [M0 + 100 * S * (i + 1) for i in range(len(ends))]
    pt = [M0 + 50 * S] + [x + d for x in t for d in (10 * S, 50 * S, 100 * S - 1)]
    pv = [partner_vals[i % len(partner_vals)] for i in range(len(pt))]
    return [span(t, ends, kind), span(pt, pv, kind if pk is None else pk)]


def double_family(name: str, kind=F64) -> RStore:
    """The stores of A.4, one group a case."""
    big = 1e308 if kind == F64 else 3e38
    sub = 5e-324 if kind == F64 else 1e-45
    cases = {
        "nan": [[1.0, NAN, 3.0], [NAN, 2.0, NAN], [NAN, NAN], [NAN, 1.0, 2.0], [1.0, 2.0, NAN], [NAN]],
        "inf": [[1.0, INF, 3.0], [-INF, 2.0], [2.0, -INF], [INF, INF], [INF, -INF]],
        "zero": [[0.0, -0.0], [-0.0, 0.0], [-0.0, -0.0, 0.0], [0.0, 0.0, -0.0]],
        "subnormal": [[sub, 3 * sub], [-sub, sub], [sub, 1.0], [0.0, sub, -0.0], [2.0 ** -1022 if kind == F64 else 2.0 ** -126, sub]],
        "diff_overflow": [[big, -big], [-big, big], [big, -big, big]],
        "prod_overflow": [[0.0, big / 1000], [big / 1000, 0.0], [0.0, -big / 1000]],
    }[name]
    series, gids = [], []
    for g, ends in enumerate(cases):
        if name == "zero":       # a partner of zeros, so that min / max / mult see nothing but zeros
            grp = _lerp_group(ends, kind, partner_vals=(-0.0, 0.0, 0.0, -0.0, 0.0))
            grp.append(span([M0 + 100 * S, M0 + 300 * S], [-0.0, 0.0] if g % 2 else [0.0, -0.0], kind))
        else:
            grp = _lerp_group(ends, kind)
        series += grp
        gids += [g] * len(grp)
    return RStore(series, gids)


DOUBLE_FAMILIES = ["nan", "inf", "zero", "subnormal", "diff_overflow", "prod_overflow"]
INF_FAMILIES = {"inf", "diff_overflow", "prod_overflow"}   # those that can hand an infinity to an aggregator


def mixed_long_store() -> RStore:
    """Integer spans at +-(2^62 + odd) in a group with one float span: isInteger is false and
    longs above 2^53 convert to double before the LERP."""
    series, gids = [], []
    for g, (a, b) in enumerate([((1 << 62) + 1, -(1 << 62) - 3), ((1 << 62) + 5, (1 << 62) + 7),
                                (-(1 << 62) - 9, (1 << 53) + 1), (LONG_MAX, LONG_MIN)]):
        grp = _lerp_group([a, b, a], LONG, pk=F64)
        grp.append(span([M0 + 150 * S, M0 + 250 * S], [(1 << 62) + 11, -(1 << 62) - 13], LONG))
        series += grp
        gids += [g] * len(grp)
    return RStore(series, gids)


def late_float_store() -> RStore:
    """Groups of integer spans and one span, not yet started for most of the window, whose first
    point is the group's only float: isInteger scans the next slot too, so every union point
    before that span starts is a double already; once the span's next point is reached and the float
    one is behind, the group's points are longs again."""
    series, gids = [], []
    for g, kind in enumerate((F32, F64)):
        clock = [M0 + 10 * S * i for i in range(200)]   # 200 union points: the late span starts in a later chunk
        series.append(span(clock, [3 * i - 100 for i in range(200)], LONG))
        series.append(span([M0 + 5 * S, M0 + 1995 * S], [1 << 40, -(1 << 40)], LONG))
        series.append([(M0 + 1500 * S, kind, 0.5), (M0 + 1700 * S, LONG, 9), (M0 + 1900 * S, LONG, -4)])
        gids += [g] * 3
    return RStore(series, gids)


WIN1 = (T0, T0 + H - 1)


# ---- A.5 rate ------------------------------------------------------------------------------------------
def _clocked(ts, vals, kinds):
    return [(t, k, v) for t, v, k in zip(ts, vals, kinds)]


def rate_store() -> RStore:
    """One group a case (two spans each, so that a rate of one span is used at the other's points)."""
    sec = [M0 + 10 * S * (i + 1) for i in range(12)]
    cases = []
    # long counters whose difference wraps
    cases.append(span(sec[:6], [LONG_MAX, LONG_MIN, LONG_MIN + 5, LONG_MAX - 1, 0, LONG_MIN], LONG))
    # values above a small counter_max, and around 2^32
    cases.append(span(sec[:8], [5000, 10, 20, (1 << 32) - 1, 3, (1 << 32) + 7, 1 << 32, 1], LONG))
    # a reset whose rate is exactly 1000 / s at counter_max 2^32 over 10 s, then one ulp above:
    # 2^32 - prev + next = 10000 and 10001
    cases.append(span(sec[:6], [100, (1 << 32) - 1000, 9000, (1 << 32) - 2000, 8001, 9000], LONG))
    # resets at the first, the last, every other point
    cases.append(span(sec[:8], [-5, 10, 20, 30, 40, 50, 60, 3], LONG))
    cases.append(span(sec[:8], [50, 10, 60, 20, 70, 30, 80, 40], LONG))
    # spans drop-resets leaves with one point and with none
    cases.append(span(sec[:2], [7, 3], LONG))
    cases.append(span(sec[:3], [-7, -8, -9], LONG))
    # double counters with NaN and infinities
    cases.append(span(sec[:8], [1.0, NAN, 3.0, 2.0, NAN, NAN, 5.0, 1.0], F64))
    cases.append(span(sec[:6], [1.0, 2.0, 4.0, 1.0, 1.5, 0.5], F32))
    # double counters a second apart at counter_max 2^32: rates equal to reset_value 1000, one ulp
    # (2^-43) above it and just below it
    cases.append(span([M0 + S * (i + 1) for i in range(6)],
                      [2.0 ** 32 - 500, 500.0, 2.0 ** 32 - 500, 500 + 2.0 ** -43, 2.0 ** 32 - 500, 500 - 2.0 ** -44], F64))
    # mixed int and float neighbours
    cases.append(_clocked(sec[:8], [10, 20.5, 15, 40, 39.5, 38, 100, 7.25], [LONG, F64, LONG, LONG, F32, LONG, LONG, F64]))
    # millisecond deltas of 1 ms
    cases.append(span([M0 + 5 * S + i for i in range(8)], [1, 3, 2, 1 << 40, 5, 4, 9, 0], LONG))
    # 65 and 129 points: prev_* and kept cross a 64-lane chunk (every third point a reset)
    for n in (65, 129):
        cases.append(span([M0 + 7 * S * (i + 1) for i in range(n)], [(i * 11) % 29 * (1 if i % 3 else -1) + 40 * i for i in range(n)], LONG))
        cases.append(span([M0 + 7 * S * (i + 1) + 1 for i in range(n)], [100 - i if i % 2 else i for i in range(n)], LONG))
    series, gids = [], []
    partner = span([M0 + 15 * S * (i + 1) for i in range(10)], [3, 9, 4, 12, 8, 30, 2, 2, 50, 1], LONG)
    for g, c in enumerate(cases):
        series += [c, partner]
        gids += [g, g]
    return RStore(series, gids)


def rate_inf_store() -> RStore:
    """Double counters with an infinity (a rate of +-Inf, or NaN from Inf - Inf) -- apart, since
    an infinite result ends the whole query."""
    sec = [M0 + 10 * S * (i + 1) for i in range(6)]
    partner = span([M0 + 15 * S * (i + 1) for i in range(4)], [3.0, 9.0, 4.0, 12.0], F64)
    series = [span(sec, [1.0, INF, INF, 2.0, -INF, 1.0], F64), partner,
              span(sec, [1.0, -INF, 3.0, 2.0, 1.0, 0.0], F64), partner]
    return RStore(series, [0, 0, 1, 1])


RATE_OPTS = [dict(), dict(counter=True), dict(counter=True, drop_resets=True),
             dict(counter=True, counter_max=1 << 32), dict(counter=True, counter_max=LONG_MAX),
             dict(counter=True, counter_max=100), dict(counter=True, counter_max=1 << 32, reset_value=1000),
             dict(counter=True, counter_max=1 << 32, reset_value=1), dict(counter=True, reset_value=5, drop_resets=True)]


# ---- A.6 strip geometry ------------------------------------------------------------------------------------
STRIP_SIZES = (1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025)


def strip_boundary(U: int) -> int:
    """The first rank of the last chunk boundary the union crosses: 512 (a k_raw_eval strip), 128
    (a k_raw_top wave) or 64 (a lane chunk); 0 when it crosses none."""
    return 512 if U > 512 else 128 if U > 128 else 64 if U > 64 else 0


def strip_store(U: int, kind) -> RStore:
    """One group whose union has exactly U points (one a second), defined by a constant-rate clock
    span; with b = strip_boundary(U): spans with points at ranks (b - 1, b), ending at b - 1,
    starting at b, a single point at rank 0 and at rank U - 1, and a span outside the scan range.
    Every span sits on the clock's timestamps, so the union stays the clock's."""
    at = lambda r: M0 + S * (r + 10)
    val = (lambda r, k: 3 * r + k) if kind == LONG else (lambda r, k: 0.25 * r + k)
    series = [span([at(r) for r in range(U)], [val(r, 0) for r in range(U)], kind)]
    b = strip_boundary(U)
    if b:
        series.append(span([at(b - 1), at(b)], [val(5, 1), val(900, 1)], kind))
        series.append(span([at(b // 3), at(b - 1)], [val(7, 2), val(-300, 2)], kind))
        series.append(span([at(b), at(U - 1)] if U - 1 > b else [at(b)], [val(-9, 3), val(40, 3)][:2 if U - 1 > b else 1], kind))
        series.append(span([at(1), at(U - 2)], [val(1000, 4), val(-1000, 4)], kind))   # LERPs across every boundary
    series.append(span([at(0)], [val(11, 5)], kind))
    series.append(span([at(U - 1)], [val(13, 6)], kind))
    series.append(span([M0 + 3 * H * S + 5 * S], [val(1, 7)], kind))   # its row lies outside the scan range
    return RStore(series, [0] * len(series))


# ---- B. the overflowing double LERP under a percentile ---------------------------------------------------------
def pct_overflow_store(sign=1.0, n_partners=299) -> RStore:
    """299 partner spans of sign * 1e306 (1 + 1e-9 j) (constant: their own LERP cannot overflow)
    and, last in the group, span A: (90 s, 0.0) .. (3540 s, sign * 1e305).  (x - x0) * 1e305 passes
    the largest double 1.8 s after A's first point, so A's operand is sign * Inf at every later
    union point before its last: the largest of 300 operands (sign +), or the smallest (sign -).

    The first partner has a point every 2 s and makes the union 1800 points long, the next twenty
    one a minute; the other 278 have two points, at 0 s and 3598 s.  A and those 278 have no point
    of their own in the union ranks 512 .. 1535: two whole strips see each of them as one window
    (m == 0), every lane of a wave takes their operand in the same step, and k_raw_top's threshold
    -- the smallest of the wave's T-th keys -- is up to date when it reaches A, the case in which
    it prunes a span without looking at its operands."""
    grid = [M0 + 60 * S * i for i in range(60)]
    clock = [M0 + 2 * S * i for i in range(1800)]
    ends = [M0, M0 + 3598 * S]
    series = []
    for j in range(n_partners):
        ts = clock if j == 0 else grid if j <= 20 else ends
        series.append(span(ts, [sign * 1e306 * (1 + 1e-9 * j)] * len(ts), F64))
    series.append(span([M0 + 90 * S, M0 + 3540 * S], [0.0, sign * 1e305], F64))
    return RStore(series, [0] * len(series))


# ---- C. missing buckets in the stores of value_edges ----------------------------------------------------------------
def sparse(store: V.Store, drop, interval_ms=60000, gids=None) -> V.Store:
    """`store` without the buckets drop[i] (bucket numbers from T0, `interval_ms` wide) of series i."""
    series = []
    for i, (ts, v, kind) in enumerate(store.series):
        gone = set(drop.get(i, ()))
        keep = [j for j, t in enumerate(ts) if (int(t) - M0) // interval_ms not in gone]
        series.append((np.asarray(ts)[keep], [v[j] for j in keep] if kind == LONG else np.asarray(v)[keep], kind))
    return V.Store(series, list(store.gids) if gids is None else gids)


def default_drop(gids, n_buckets):
    """Per group: its first series loses bucket 4 (between two present ones; in the stores with a
    NaN or infinite bucket 3 the neighbour is that bucket) and, over several hours, bucket 64; its
    second series the first bucket; its third (or, in a group of two, the first again) the last."""
    drop = {}
    for g in sorted(set(gids)):
        mem = [i for i, x in enumerate(gids) if x == g]
        if len(mem) < 2:
            continue
        drop[mem[0]] = {4} | ({64} if n_buckets > 65 else set())
        drop[mem[1]] = {0}
        drop.setdefault(mem[2] if len(mem) > 2 else mem[0], set()).add(n_buckets - 1)
        drop[mem[0]] = set(drop[mem[0]])
    return drop


def sparse_stores():
    """name -> (factory, window): the stores of C in the one_row (K = 60) and rows (K = 180) shapes
    under 1m buckets."""
    out = {}
    for shape in ("one_row", "rows"):
        rows = V.SHAPES[shape][0]
        K = rows * 60
        win = (T0, T0 + rows * H - 1)
        base = {
            "zeros f64 +": (lambda shape=shape: V.zeros_store(F64, 1.0, shape), [0, 0, 1, 1]),
            "zeros f32 -": (lambda shape=shape: V.zeros_store(F32, -1.0, shape), [0, 0, 0, 0]),
            "zero groups +--+-": (lambda shape=shape: V.zero_groups_store([1, -1, -1, 1, -1], shape=shape), None),
            "zero groups -++": (lambda shape=shape: V.zero_groups_store([-1, 1, 1], F32, shape=shape), None),
            "nan bucket f32": (lambda shape=shape: V.nan_store("bucket", F32, shape), None),
            "nan bucket f64": (lambda shape=shape: V.nan_store("bucket", F64, shape), None),
            "inf +": (lambda shape=shape: V.inf_store((1,), F64, shape), None),
            "inf -": (lambda shape=shape: V.inf_store((-1,), F32, shape), None),
            "inf +-": (lambda shape=shape: V.inf_store((1, -1), F64, shape), None),
            "overflow": (lambda shape=shape: V.overflow_store(shape), None),
            "scaled -1060": (lambda shape=shape: V.scaled_store(-1060, shape=shape), None),
            "scaled 0": (lambda shape=shape: V.scaled_store(0, shape=shape), None),
            "scaled 960": (lambda shape=shape: V.scaled_store(960, shape=shape), None),
            "longs": (lambda shape=shape: V.long_store(shape=shape), None),
        }
        for name, (make, gids) in base.items():
            def factory(make=make, gids=gids, K=K):
                st = make()
                g = list(st.gids) if gids is None else gids
                return sparse(st, default_drop(g, K), gids=g)
            out[f"{name}/{shape}"] = (factory, win)
    return out


def slot_facts(store: V.Store, interval_ms=60000):
    """(interpolated, absent at an end): the numbers of (series, slot) pairs whose bucket is missing
    while the group has the slot, between two present buckets of the series / before its first or
    after its last."""
    interp = absent = 0
    have = [set(V.buckets_of(ts, v, interval_ms)) for ts, v, _ in store.series]
    for i, g in enumerate(store.gids):
        group = set().union(*[have[j] for j, x in enumerate(store.gids) if x == g])
        for b in group - have[i]:
            if min(have[i]) < b < max(have[i]):
                interp += 1
            else:
                absent += 1
    return interp, absent


# ---- the cases: name -> (store factory, window, aggregators, rate options or None) ----------------------------------
WIN2 = (T0, T0 + 2 * H - 1)
A_AGGS = ["sum", "min", "max", "avg", "dev", "mult", "none"]
VALUE_AGGS = A_AGGS + ["first", "last", "count"]
PCT_AGGS = ["p50", "median", "p90", "p99", "p999", "ep99r7"]
RATE_AGGS = ["sum", "min", "max", "avg", "dev", "none"]
KIND_NAMES = {F64: "f64", F32: "f32", LONG: "int"}

RAW_CASES = {}
for _den in WINDOW_DENS:
    RAW_CASES[f"window/{_den}"] = (lambda den=_den: window_store(den), WIN2, A_AGGS, None)
RAW_CASES["jdiv"] = (jdiv_store, WIN1, A_AGGS, None)
for _fam in DOUBLE_FAMILIES:
    for _kind in (F64, F32):
        RAW_CASES[f"double/{_fam}/{KIND_NAMES[_kind]}"] = (lambda f=_fam, k=_kind: double_family(f, k), WIN1, VALUE_AGGS, None)
RAW_CASES["double/mixed_long"] = (mixed_long_store, WIN1, VALUE_AGGS, None)
RAW_CASES["double/late_float"] = (late_float_store, WIN1, VALUE_AGGS, None)
for _U in STRIP_SIZES:
    for _kind in (LONG, F64):
        RAW_CASES[f"strip/{_U}/{KIND_NAMES[_kind]}"] = (lambda U=_U, k=_kind: strip_store(U, k), WIN1, A_AGGS, None)
RAW_CASES["rate"] = (rate_store, WIN1, RATE_AGGS, RATE_OPTS)
RAW_CASES["rate_inf"] = (rate_inf_store, WIN1, RATE_AGGS, RATE_OPTS[:3])

# B: the double families and the integer windows under the percentile aggregators
PCT_CASES = {n: (c[0], c[1]) for n, c in RAW_CASES.items() if n.startswith(("double/", "window/"))}
PCT_CASES["pct_overflow/+"] = (lambda: pct_overflow_store(1.0), WIN1)
PCT_CASES["pct_overflow/-"] = (lambda: pct_overflow_store(-1.0), WIN1)


def queries_of(name):
    """[(label, query)] of a case of RAW_CASES."""
    _, win, aggs, rates = RAW_CASES[name]
    if rates is None:
        return [(a, abi.new_query(win[0], win[1], a)) for a in aggs]
    return [(f"{a} {o}", abi.new_query(win[0], win[1], a, rate=True, **o)) for o in rates for a in aggs]


def pct_queries_of(name):
    win = PCT_CASES[name][1]
    return [(a, abi.new_query(win[0], win[1], a)) for a in PCT_AGGS]
