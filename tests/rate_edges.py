"""Helpers of the edge tests of the rate over downsampled buckets (test_rate_edges_cpu.py,
test_gpu_rate_edges.py): RateSpan over the bucket stream, the rate branch of emit_series_to
(opentsdb_amd/csrc/kcommon.h).

* ref_ds_rate_query: a plain Python restatement of a downsampled (rate) query -- the scan range
  (TsdbQuery.getScanStartTimeSeconds / getScanEndTimeSeconds), the fixed-interval buckets of
  Downsampler (src/core/Downsampler.java: the seek to the first interval boundary at or after
  the scan start, ValuesInInterval) and the grid of FillingDownsampler
  (src/core/FillingDownsampler.java: from the boundary at or before the scan start to the one
  at or before the scan end), then raw_edges.rate_span and raw_edges.aggregate.  Python floats
  stand for Java doubles; no numpy in the arithmetic.  A third leg beside the engine and the C
  oracle.
* builders of small stores whose buckets sit where the rate branch can go wrong:
  a. the 64-lane chunk geometry (resets, first points, whole chunks without a survivor or without
     an item at the chunk boundaries), for K slots of one point each;
  b. counter arithmetic on buckets (roll-over from the pseudo-point (0, 0L), counter_max,
     reset_value ties, dropped resets, signed zeros, infinities, NaN buckets, fill policies);
  c. the K thresholds of the routes, restated from the LDS formulas of the kernels.
"""
from __future__ import annotations

import math

import numpy as np

from opentsdb_amd import abi
from tests import raw_edges as R
from tests import value_edges as V

T0, H, M0 = R.T0, R.H, R.M0
LONG, F32, F64 = R.LONG, R.F32, R.F64
NAN, INF = R.NAN, R.INF
FILLS = {"none": abi.FILL_NONE, "nan": abi.FILL_NAN, "zero": abi.FILL_ZERO, "null": abi.FILL_NULL,
         "scalar": abi.FILL_SCALAR}


# ---- the third leg ----------------------------------------------------------------------------------
def scan_bounds(q):
    """TsdbQuery's scan range in seconds of a query with a fixed-interval downsampler (second
    timestamps): the start aligned down to the interval, then to the hour row; the end moved to
    the next interval boundary, then up to an hour."""
    I = q.ds_interval_ms
    s, e = q.start_time, q.end_time
    assert s < (1 << 32) and e < (1 << 32) and I > 0
    a = s - ((1000 * s) % I) // 1000
    ss = max(a - a % 3600, 0)
    ia = e + (I - (1000 * e) % I) // 1000
    return ss, ia if ia % 3600 == 0 else ia + 3600 - ia % 3600


def buckets(pts, fn, I, ss_ms):
    """Downsampler over the points [(ts, is_int, value)] of a span after AggregationIterator's
    seek to the scan start: Downsampler.seek moves the source to the first interval boundary at
    or after it (points before that boundary are gone), ValuesInInterval hands every value out
    as a double and the downsample function's runDouble skips NaN as it does anywhere."""
    seek = (ss_ms + I - 1) // I * I
    out = {}
    for t, _, v in pts:
        if t >= seek:
            out.setdefault(t - t % I, []).append(float(v))
    return {b: R.run_double(fn, vals) for b, vals in out.items()}


def ds_stream(pts, fn, I, fill, ss_ms, se_ms):
    """([(ts, False, value)], gap): the stream the span's downsampler hands to RateSpan or to the
    aggregator.  Fill NONE: the buckets that hold a point.  Any other policy: FillingDownsampler's
    grid from align(scan start) up to, not including, align(scan end), whatever the span holds; a
    missing bucket is NaN (NAN, NULL), 0.0 (ZERO) or, under SCALAR, an error (gap: the stream then
    holds NaN there and the caller raises)."""
    b = buckets(pts, fn, I, ss_ms)
    if fill == abi.FILL_NONE:
        return [(t, False, b[t]) for t in sorted(b)], False
    out, gap = [], False
    t, end = ss_ms - ss_ms % I, se_ms - se_ms % I
    while t < end:
        if t in b:
            out.append((t, False, b[t]))
        else:
            gap = gap or fill == abi.FILL_SCALAR
            out.append((t, False, 0.0 if fill == abi.FILL_ZERO else NAN))
        t += I
    return out, gap


def ref_ds_rate_query(store: R.RStore, q):
    """The downsampled query (with or without rate) on the Python reference: [(group id, ts, bits,
    is_int)] as oracle.run_query returns it, or RefError with the Java exception's name.  The
    groups run in order and the first one that raises ends the query.  A group with a FILL_SCALAR
    gap raises RuntimeException; a group that would raise for an infinity as well is refused
    (which of the two comes first depends on how far the iterators have read ahead)."""
    assert q.ds_function >= 0 and q.ds_interval_ms > 0 and not q.ds_all and not q.ds_calendar
    name, fn = abi.AGGREGATOR_NAMES[q.aggregator], abi.AGGREGATOR_NAMES[q.ds_function]
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
    for gid, members in groups:
        views, gap = [], False
        for pts in members:
            v, g = ds_stream(pts, fn, q.ds_interval_ms, q.ds_fill, ss * 1000, se * 1000)
            gap = gap or g
            if q.rate:
                v = R.rate_span(v, bool(q.rate_counter), q.rate_counter_max, q.rate_reset_value, bool(q.rate_drop_resets))
            views.append(v)
        try:
            pts = R.aggregate(views, ss * 1000, se * 1000, name, abi.interpolation_of(q.aggregator), bool(q.rate))
        except R.RefError:
            assert not gap, "a FILL_SCALAR gap and an infinity in one group: the order is not restated"
            raise
        if gap:
            raise R.RefError("RuntimeException")
        out.append((gid, np.array([p[0] for p in pts], np.int64),
                    np.array([(p[2] & ((1 << 64) - 1)) if p[1] else R.dbits(p[2]) for p in pts], np.uint64),
                    np.array([1 if p[1] else 0 for p in pts], np.uint8)))
    return out


def ref_outcome(store, q):
    try:
        return ref_ds_rate_query(store, q), None
    except R.RefError as e:
        return None, e.java


# ---- the slot grid of a query, as the planner has it ----------------------------------------------------
def slots(win, I, fill=abi.FILL_NONE):
    """(B0, K) of a fixed-interval downsampled query: slot 0 starts at the first interval boundary at
    or after the scan start; fill NONE has a slot for every bucket that starts before the scan end,
    a fill policy stops at the boundary at or before it (plan_query in csrc/engine.cpp)."""
    ss, se = scan_bounds(abi.new_query(win[0], win[1], "sum", ds_function=abi.AGG["sum"], ds_interval_ms=I))
    S0, E0 = ss * 1000, se * 1000
    B0 = (S0 + I - 1) // I * I
    if fill != abi.FILL_NONE:
        return B0, max((E0 - E0 % I - B0) // I, 0)
    return B0, max((E0 - B0 + I - 1) // I, 0)


def interval_for(K, win):
    """An interval (ms) that gives the window K slots under fill NONE: the one that divides the
    scanned span where there is one, else the widest that fits."""
    ss, se = win[0] - win[0] % 3600, win[1] + 3600 - win[1] % 3600
    span = (se - ss) * 1000
    if span % K == 0 and slots(win, span // K)[1] == K:
        return span // K
    for I in range(span // max(K - 1, 1), span // (K + 1), -1):
        if slots(win, I)[1] == K:
            return I
    raise ValueError(K)


def query(win, agg, fn, I, fill="none", rate=None):
    kw = {} if rate is None else dict(rate=True, **rate)
    return abi.new_query(win[0], win[1], agg, ds_function=abi.AGG[fn], ds_interval_ms=I, ds_fill=FILLS[fill], **kw)


# ---- a. chunk geometry -----------------------------------------------------------------------------------
GEOMETRY_K = (1, 2, 3, 63, 64, 65, 127, 128, 129, 193)
RESET_SLOTS = (1, 2, 62, 63, 64, 65, 127, 128)
# one scanned hour row, and three ("several one-chunk rows"), for every interval up to an hour: the
# start lies more than an interval inside the first row (aligned down to the interval it stays in
# that row), the end more than an interval before the end of the last
WIN_A = (T0 + 200, T0 + H - 200)
WIN_A3 = (T0 + 200, T0 + 3 * H - 200)


class Geometry:
    """A family-a store: K slots, one point a bucket (at the bucket's start, a millisecond later
    where that keeps a millisecond interval off the whole second), spans by name."""

    def __init__(self, K, win=WIN_A, I=None):
        self.K, self.win = K, win
        self.I = I = interval_for(K, win) if I is None else I
        assert slots(win, I)[1] == K
        self.B0 = B0 = slots(win, I)[0]
        self.at = lambda k: B0 + k * I + (1 if I % 1000 and (B0 + k * I) % 1000 == 0 else 0)
        self.spans = {}     # name -> ([slot], [value], kind, group)
        hi = K - 1
        resets = {s for s in RESET_SLOTS + (hi,) if 1 <= s <= hi}
        self.add("resets", range(K), self.counter(range(K), resets, 1000, 10, 7), LONG, 0)
        self.add("resets f32", range(K), [0.5 * v for v in self.counter(range(K), resets, 300, 4, 9)], F32, 2)
        for name, first, g in (("first 63", min(63, hi), 0), ("first 64", min(64, hi), 1), ("first K-1", hi, 2)):
            sl = range(first, K)
            self.add(name, sl, self.counter(sl, {first + 2}, 100, 3, 50), LONG, g)
        # 64 or more resets in a row: from slot lo to slot hi2 the values fall (K >= 129: the whole
        # chunk 64 .. 127 has no survivor under drop_resets), before and after they rise
        lo, hi2 = min(max(1, K // 4), 30), min(hi, 135)
        v, vals = 0.0, []
        for k in range(K):
            v = 2.25 * k if k < lo else v - 1.0 if k <= hi2 else v + 1.5
            vals.append(v + (5000.5 if k == lo else 0.0))
            v = vals[-1]
        self.add("long reset", range(K), vals, F64, 1)
        self.long_reset = (lo, hi2)
        # two points more than 64 slots apart (K >= 129: the chunk between them holds no item)
        far = 128 if K == 129 else 140 if K > 140 else min(68, hi)
        self.add("gap", [min(2, max(hi - 1, 0)), far], [40, 75], LONG, 0)
        self.add("one point", [min(5, hi)], [2.5], F32, 1)
        self.add("two points", [min(3, max(hi - 1, 0)), min(4, hi)], [7, 19], LONG, 1)
        # under counter and drop_resets: the first rate (against (0, 0L)) is dropped, the second
        # survives, every later one is dropped
        n = min(K, 70)
        self.add("second only", range(n), [-5, 100] + [99 - i for i in range(n - 2)], LONG, 2)
        # the same, and a second survivor two chunks later (K = 193: slot 131), contributed to every
        # slot before it
        last_fall = min(hi - 1, 130)
        vals = [-5, 100] + [99 - i for i in range(K - 2)]
        for k in range(last_fall + 1, K):
            vals[k] = 1000 + 3 * k
        self.add("late second", range(K), vals[:K], LONG, 2)
        names = list(self.spans)
        self.store = R.RStore([R.span([self.at(k) for k in s[0]], s[1], s[2]) for s in self.spans.values()],
                              [s[3] for s in self.spans.values()])
        order = sorted(range(len(names)), key=lambda i: self.spans[names[i]][3])
        self.names = [names[i] for i in order]      # in the store's series order

    @staticmethod
    def counter(sl, resets, start, up, down):
        v, out = start, []
        for i, k in enumerate(sl):
            if i:
                v = v - down if k in resets else v + up
            out.append(v)
        return out

    def add(self, name, sl, vals, kind, group):
        sl = list(sl)
        keep = [i for i, k in enumerate(sl) if 0 <= k < self.K and k not in sl[:i]]
        self.spans[name] = ([sl[i] for i in keep], [vals[i] for i in keep], kind, group)

    def stream_slots(self, name, q):
        """The slots of the bucket stream the span hands to RateSpan, and the stream."""
        i = self.names.index(name)
        ss, se = scan_bounds(q)
        pts = [(t, k == LONG, v) for t, k, v in self.store.series[i]]
        st, _ = ds_stream(pts, abi.AGGREGATOR_NAMES[q.ds_function], q.ds_interval_ms, q.ds_fill, ss * 1000, se * 1000)
        return [(p[0] - self.B0) // self.I for p in st], st

    def survivors(self, name, q):
        """The slots whose rate RateSpan hands out (the rates that are not dropped)."""
        sl, st = self.stream_slots(name, q)
        kept = R.rate_span(st, bool(q.rate_counter), q.rate_counter_max, q.rate_reset_value, bool(q.rate_drop_resets))
        return [(p[0] - self.B0) // self.I for p in kept]


# rate option sets of families a and b: raw_edges.RATE_OPTS, and the reset_value ties of rate_tie()
TIE_MAX, TIE_RESET = 1 << 32, 1000
RATE_OPTS = R.RATE_OPTS + [dict(counter=True, counter_max=TIE_MAX, reset_value=TIE_RESET, drop_resets=True),
                           dict(counter=True, counter_max=TIE_MAX, reset_value=TIE_RESET - 1),
                           dict(counter=True, counter_max=TIE_MAX, reset_value=TIE_RESET + 1)]
A_OPTS = [R.RATE_OPTS[i] for i in (0, 1, 2, 6, 8)]
EXACT_AGGS = ("none", "max", "min", "count", "p50", "p99")    # compared bit for bit
TOL_AGGS = ("sum", "avg", "dev")                              # REL_TOL, REL_TOL, DEV_TOL
A_FILLS = ("none", "nan", "zero")


def opt_label(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "plain"


def geometry_queries(geo: Geometry):
    """[(label, aggregator, rate options, query)]: sum downsampling (one point a bucket) under
    every fill x option set x aggregator, and max / count / last downsampling under two."""
    out = []
    for fill in A_FILLS:
        for o in A_OPTS:
            for agg in EXACT_AGGS + TOL_AGGS:
                out.append((f"{agg}:sum fill {fill} {opt_label(o)}", agg, o, query(geo.win, agg, "sum", geo.I, fill, o)))
    for fn in ("max", "count", "last"):
        for o in (A_OPTS[1], A_OPTS[2]):
            for agg in ("none", "sum"):
                out.append((f"{agg}:{fn} fill none {opt_label(o)}", agg, o, query(geo.win, agg, fn, geo.I, "none", o)))
    return out


GEOMETRY_CASES = {f"K{K}": (lambda K=K: Geometry(K)) for K in GEOMETRY_K}
GEOMETRY_CASES["K193/3h"] = lambda: Geometry(193, WIN_A3)
GEOMETRY_CASES["110s"] = None    # (filled in below: 110 s buckets, which do not divide the hour)


class Geometry110(Geometry):
    """110 s buckets over two hour rows: the interval divides neither the hour nor the scan start,
    so the Downsampler's seek drops the points before the first boundary and FillingDownsampler's
    grid starts one bucket before slot 0."""

    def __init__(self):
        win = (T0 + 200, T0 + 2 * H - 200)    # (a start inside the first 110 s would scan the hour before)
        super().__init__(slots(win, 110000)[1], win, 110000)
        # a point between the scan start and the first boundary: gone after the seek
        i = self.names.index("gap")
        self.store = R.RStore([s + [] if j != i else [(M0 + 1000, LONG, 3)] + s for j, s in enumerate(self.store.series)],
                              self.store.gids)


GEOMETRY_CASES["110s"] = Geometry110


def nocert_geometry() -> Geometry:
    """The K = 129 store with every value v as the float64 2^52 + 1 + 2 round(4 v) (odd, rising with
    v: the resets stay where they are): 129 of them add to far more than a double holds exactly, so
    every row is past the exactness certificate and the sequential dense kernels take the scan."""
    geo = Geometry(129)
    geo.store = R.RStore([[(t, F64, float((1 << 52) + 1 + 2 * round(4 * v))) for t, _, v in s] for s in geo.store.series],
                         geo.store.gids)
    return geo


# ---- b. counter arithmetic on buckets ------------------------------------------------------------------------
I_B = 60000
WIN_B = (T0, T0 + H - 1)     # K = 60


def rate_tie(dt_s=I_B // 1000, counter_max=TIE_MAX, target=float(TIE_RESET)):
    """Buckets (v0, [v1 ...]) of a double counter whose roll-over rate (counter_max - v0 + v1) / dt
    is exactly the reset value, the next double above it and the next one below it."""
    v0 = float(counter_max) - 50000.0
    base = target * dt_s - 50000.0
    step = math.ulp(target * dt_s)
    want = [target, math.nextafter(target, INF), math.nextafter(target, 0.0)]
    out = []
    for w, sg in zip(want, (0, 1, -1)):
        for j in range(0, 200):
            v1 = base + sg * j * step
            if (float(counter_max) - v0 + v1) / float(dt_s) == w:
                out.append(v1)
                break
        else:
            raise ValueError(w)
    return v0, out


def _minutes(vals, kind, first=1, per_bucket=1):
    """Points of the buckets first, first + 1 ... (60 s wide); per_bucket points a bucket, the
    bucket's value split among them (so that sum downsampling restores it)."""
    ts, out = [], []
    for i, v in enumerate(vals):
        for j in range(per_bucket):
            ts.append(M0 + (first + i) * I_B + j * 10 * R.S)
            out.append(v if j == 0 or v != v else 0 if kind == LONG else 0.0)
    return R.span(ts, out, kind)


def counter_cases():
    """name -> [spans] (one group a case)."""
    v0, (eq, up, dn) = rate_tie()
    c = {}
    c["negative first"] = [_minutes([-5, 10, 20, 15, 40], LONG), _minutes([-2.5, 1.0, 0.5], F64, first=2)]
    c["long max"] = [_minutes([R.LONG_MAX, 5, R.LONG_MAX - 7, R.LONG_MIN, 0], LONG), _minutes([9e18, 1.0, 9e18], F64)]
    c["above counter_max"] = [_minutes([5000, 10, 20, (1 << 32) + 7, 3, 1 << 33, 1], LONG)]
    c["tie"] = [_minutes([v0, eq, v0, up, v0, dn, v0, eq], F64)]
    c["tie ints"] = [_minutes([TIE_MAX - 50000, 10000, TIE_MAX - 50000, 10001, TIE_MAX - 50000, 9999], LONG)]
    c["dropped is previous"] = [_minutes([10, 5, 7, 6, 6, 20], LONG, per_bucket=3), _minutes([1.5, 0.5, 0.75, 0.25], F32, first=2)]
    c["zero diffs"] = [_minutes([1.5, 1.5, 0.0, -0.0, -0.0, 0.0, 0.0], F64), _minutes([-0.0, -0.0, 0.0], F32, first=1)]
    c["nan buckets"] = [_minutes([1.0, NAN, 3.0, 2.0, NAN, NAN, 5.0, 1.0], F64, per_bucket=2), _minutes([NAN, NAN, 4.0, NAN], F32)]
    c["gaps"] = [R.span([M0 + k * I_B for k in (1, 2, 5, 6, 9, 40)], [10, 20, 30, 25, 50, 60], LONG),
                 R.span([M0 + k * I_B for k in (3, 5, 30)], [1.5, 2.5, 0.5], F64)]
    c["mixed kinds"] = [R._clocked([M0 + k * I_B for k in range(1, 9)], [10, 20.5, 15, 40, 39.5, 38, 100, 7.25],
                                   [LONG, F64, LONG, LONG, F32, LONG, LONG, F64])]
    return c


def counter_store() -> R.RStore:
    series, gids = [], []
    for g, spans in enumerate(counter_cases().values()):
        series += spans
        gids += [g] * len(spans)
    return R.RStore(series, gids)


def full_store() -> R.RStore:
    """Two groups whose spans hold every bucket of the hour (no fill policy finds a gap), group 1
    with a reset in every other bucket."""
    ts = [M0 + k * I_B for k in range(60)]
    return R.RStore([R.span(ts, [10 * k for k in range(60)], LONG), R.span(ts, [0.5 * k for k in range(60)], F64),
                     R.span(ts, [100 + (k % 2) * 50 - k for k in range(60)], LONG)], [0, 0, 1])


def inf_store(first: str) -> R.RStore:
    """Two groups: "inf" holds a double counter whose difference overflows (1e308 after -1e308 and
    back), "gap" a span with missing buckets; `first` names the one with the smaller group id."""
    ts = [M0 + k * I_B for k in range(60)]
    inf = [R.span(ts, [(-1e308 if k == 7 else 1e308 if k in (8, 20) else -1e308 if k == 21 else 1.0) for k in range(60)], F64),
           R.span(ts, [2.0] * 60, F64)]
    gap = [R.span(ts[:10] + ts[12:], [3 * k for k in range(58)], LONG)]
    order = [inf, gap] if first == "inf" else [gap, inf]
    return R.RStore(order[0] + order[1], [0] * len(order[0]) + [1] * len(order[1]))


COUNTER_CASES = {"counter": counter_store, "full": full_store, "inf first": lambda: inf_store("inf"),
                 "gap first": lambda: inf_store("gap")}
B_FILLS = {"counter": ("none", "nan", "zero", "null", "scalar"), "full": ("none", "zero", "scalar"),
           "inf first": ("none", "zero", "scalar"), "gap first": ("none", "nan", "scalar")}
B_FUNS = {"counter": ("sum", "avg", "min", "max", "count", "first", "last"), "full": ("sum",),
          "inf first": ("sum",), "gap first": ("sum",)}


def counter_queries(name):
    """[(label, aggregator, rate options, query)] of a family-b store: every option set under sum
    downsampling x fill x aggregator, the other downsample functions under two option sets."""
    out = []
    for fill in B_FILLS[name]:
        for o in RATE_OPTS:
            for agg in EXACT_AGGS + TOL_AGGS:
                if fill in ("null", "scalar") and agg in ("p50", "p99", "dev", "avg"):
                    continue
                out.append((f"{agg}:sum fill {fill} {opt_label(o)}", agg, o, query(WIN_B, agg, "sum", I_B, fill, o)))
    for fn in B_FUNS[name][1:]:
        for o in (RATE_OPTS[1], RATE_OPTS[2]):
            for agg in ("none", "sum", "max"):
                out.append((f"{agg}:{fn} fill none {opt_label(o)}", agg, o, query(WIN_B, agg, fn, I_B, "none", o)))
    return out


def precedence_queries():
    """[(label, aggregator, query)] under FILL_SCALAR over the stores of inf_store: one group raises
    IllegalStateException ("Got Infinity"), the other RuntimeException (a missing bucket); the
    reference hands out the exception of the group that comes first."""
    return [(f"{agg}:sum fill scalar {opt_label(o)}", agg, query(WIN_B, agg, "sum", I_B, "scalar", o))
            for o in (RATE_OPTS[0], RATE_OPTS[1], RATE_OPTS[2]) for agg in ("none", "sum", "max", "count")]


def lead_store() -> R.RStore:
    """Two spans with a point in every 110 s bucket of Geometry110's window and one before slot 0:
    no slot of a fill policy's grid is missing but the one before slot 0, which the seek emptied."""
    geo = Geometry110()
    ts = [M0 + 1000] + [geo.at(k) for k in range(geo.K)]
    return R.RStore([R.span(ts, [3 * i for i in range(len(ts))], LONG), R.span(ts, [0.5 * i for i in range(len(ts))], F64)], [0, 0])


def lead_queries():
    geo = Geometry110()
    return [(f"{agg}:sum fill {fill} {opt_label(o)}", agg, query(geo.win, agg, "sum", geo.I, fill, o))
            for fill in ("scalar", "zero", "nan") for o in (RATE_OPTS[0], RATE_OPTS[2]) for agg in ("none", "sum", "max")]


# ---- c. the K thresholds of the routes ---------------------------------------------------------------------------
# LDS bytes a wave takes, restated from csrc/kcommon.h (fast_slot_bytes, slot_lds_bytes,
# fixed_lds_bytes; VBUF = 4224, CH = 512) and csrc/k_misc.hip (fast_wave_lds, grid_wave_lds):
#   fast_wave_lds(K, rate, part) = a16(1024 + a16(8K) + a16(4K) + a16(K) + [rate] a16(8K)
#                                      + [part] (2 a16(8K) + 2 a16(4K)))     ~ 1024 + 37 K (+ 8 K)
#   grid_wave_lds(K, rate, false) = a16(fixed + a16(8K) + a16(K) + [rate] a16(8K) + 2 a16(8K) + 2 a16(4K))
#   fixed = VBUF + 4 CH + a16(2 (CH + 1)) = 7312
# The fused streaming pass takes a query while fast_wave_lds(K, rate, true) <= 32 KB
# (dense_split_wanted in csrc/engine.cpp): K <= 705 with rate, K <= 857 without; above it the dense
# split writes the buckets to HBM and k_emit works over them.  k_grid keeps its slots in LDS while
# grid_wave_lds(K, rate, false) <= 40 KB (plan_query: P.gslot): K <= 820 with rate.  The constants
# below are computed from the formulas; test_rate_edges_cpu.py compares VBUF and CH with the header.
VBUF, CH = 4224, 512


def a16(x):
    return (x + 15) & ~15


def fast_slot_bytes(K, rate, part=True):
    return a16(K * 8) + a16(K * 4) + a16(K) + (a16(K * 8) if rate else 0) + (a16(K * 8) * 2 + a16(K * 4) * 2 if part else 0)


def fast_wave_lds(K, rate, part=True):
    return a16(1024 + fast_slot_bytes(K, rate, part))


def fixed_lds_bytes():
    return VBUF + CH * 4 + ((CH + 1) * 2 + 15) // 16 * 16


def slot_lds_bytes(K, rate):
    return a16(K * 8) + a16(K) + (a16(K * 8) if rate else 0) + a16(K * 8) * 2 + a16(K * 4) * 2


def grid_wave_lds(K, rate, gslot=False):
    return a16(fixed_lds_bytes() + (0 if gslot else slot_lds_bytes(K, rate)))


def last_k(fits):
    """The largest K the (monotone) budget admits."""
    K = 1
    while fits(K + 1):
        K += 1
    return K


K_FUSED_RATE = last_k(lambda K: fast_wave_lds(K, True) <= 32 * 1024)
K_FUSED = last_k(lambda K: fast_wave_lds(K, False) <= 32 * 1024)
K_GRID_LDS = last_k(lambda K: grid_wave_lds(K, True) <= 40 * 1024)
K_DAY = 1440
THRESHOLD_K = sorted({K_FUSED_RATE, K_FUSED_RATE + 1, K_GRID_LDS, K_GRID_LDS + 1, K_FUSED, K_FUSED + 1, K_DAY})
THRESHOLD_SHAPES = {"rows": 4, "walker": 1}     # hour rows scanned


def threshold_store(shape) -> R.RStore:
    """Four series in two groups, 1440 points each, counters with a reset every 97th point, small
    multiples of 0.25 (every bucket sum is exact in any order) in float32 (rows) or float64
    (walker) cells.
    rows: a point every 10 s over four hour rows of 360 points (one-chunk rows); walker: a point
    every 2.5 s in one hour row of 1440 points (over one chunk of 512), on millisecond qualifiers."""
    if shape == "rows":
        ts = [M0 + 10 * R.S * i for i in range(1440)]
    else:
        ts = [M0 + 2500 * i + 1 for i in range(1440)]
    series = []
    for s in range(4):
        kind = F32 if shape == "rows" else F64
        v, vals = 50 * s, []
        for i in range(1440):
            v = (i * 7 + s) % 23 if (i + 11 * s) % 97 == 96 else v + 1 + (i * (s + 3)) % 5
            vals.append(v if kind == LONG else 0.25 * v)
        series.append(R.span(ts, vals, kind))
    return R.RStore(series, [0, 0, 1, 1])


def threshold_window(shape):
    return (T0 + 200, T0 + THRESHOLD_SHAPES[shape] * H - 200)


def threshold_queries(shape, K):
    """[(label, query)]: the rate query (counter with drop_resets, and plain), and its twin
    without rate, at the interval that gives the window K slots."""
    win = threshold_window(shape)
    I = interval_for(K, win)
    assert slots(win, I)[1] == K
    out = []
    for agg in ("sum", "max"):
        out.append((f"{agg} rate counter drop", query(win, agg, "sum", I, "none", dict(counter=True, drop_resets=True))))
        out.append((f"{agg} rate", query(win, agg, "sum", I, "none", {})))
        out.append((f"{agg} no rate", query(win, agg, "sum", I)))
    return out


def compare(agg, rel_tol, dev_tol):
    """The comparator of an aggregator: bits, or the project's tolerance of sum / avg and of dev."""
    if agg in EXACT_AGGS:
        return V.assert_bits
    tol = dev_tol if agg == "dev" else rel_tol
    return lambda g, w, c="": V.assert_rel(g, w, tol, c)
