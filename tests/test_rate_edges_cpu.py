"""The stores of the rate-over-buckets edge tests are what they claim to be, and the plain Python
restatement of a downsampled rate query (tests/rate_edges.py: the scan range, Downsampler,
FillingDownsampler's grid, then raw_edges.rate_span and raw_edges.aggregate) equals the C oracle on
every store and query of tests/test_gpu_rate_edges.py: the same groups, timestamps and Java
exception, the same bits under none / max / min / count / p50 / p99, REL_TOL under sum / avg, DEV_TOL
under dev.  No GPU."""
from __future__ import annotations

import math
import os
import re

import numpy as np
import pytest

from opentsdb_amd import abi
from oracle import oracle as O
from tests import rate_edges as X
from tests import raw_edges as R

REL_TOL, DEV_TOL = 1e-12, 1e-9    # the project's tolerances (tests/test_gpu_parity.py)


def oracle_outcome(batch, q):
    try:
        return O.run_query(batch, q), None
    except O.OracleError as e:
        return None, e.java


def assert_ref_is_oracle(store, q, agg, ctx):
    assert X.scan_bounds(q) == O.scan_bounds(q), f"{ctx}: scan range"
    want, ref = oracle_outcome(store.batch, q), X.ref_outcome(store, q)
    assert ref[1] == want[1], f"{ctx}: the Python reference raised {ref[1]}, the oracle {want[1]}"
    if want[1] is None:
        X.compare(agg, REL_TOL, DEV_TOL)(ref[0], want[0], ctx)
    return want


@pytest.fixture(scope="module")
def geos():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = X.GEOMETRY_CASES[name]()
        return cache[name]
    return get


def test_tolerances_are_the_projects():
    from tests import test_gpu_parity as P
    assert (REL_TOL, DEV_TOL) == (P.REL_TOL, P.DEV_TOL)


# ---- the Python reference against the oracle --------------------------------------------------------
@pytest.mark.parametrize("name", list(X.GEOMETRY_CASES))
def test_reference_equals_oracle_geometry(geos, name):
    geo = geos(name)
    assert len(geo.store.series) <= 16 and max(len(s) for s in geo.store.series) <= 1500
    for label, agg, _, q in X.geometry_queries(geo):
        assert_ref_is_oracle(geo.store, q, agg, f"{name} {label}")


@pytest.mark.parametrize("name", list(X.COUNTER_CASES))
def test_reference_equals_oracle_counter(name):
    st = X.COUNTER_CASES[name]()
    assert len(st.series) <= 16
    for label, agg, _, q in X.counter_queries(name):
        assert_ref_is_oracle(st, q, agg, f"{name} {label}")


@pytest.mark.parametrize("first", ["inf", "gap"])
def test_reference_equals_oracle_scalar_precedence(first):
    st = X.inf_store(first)
    errs = set()
    for label, agg, q in X.precedence_queries():
        errs.add(assert_ref_is_oracle(st, q, agg, f"{first} first {label}")[1])
    # (count absorbs the infinity: with the gap group second the query still raises for the gap)
    assert errs == ({"IllegalStateException", "RuntimeException"} if first == "inf" else {"RuntimeException"})


def test_reference_equals_oracle_leading_fill_bucket():
    """Every slot of the grid holds a point, yet FILL_SCALAR raises: the bucket before slot 0."""
    st = X.lead_store()
    for label, agg, q in X.lead_queries():
        want = assert_ref_is_oracle(st, q, agg, f"lead {label}")
        assert (want[1] == "RuntimeException") == (q.ds_fill == abi.FILL_SCALAR)


def test_reference_equals_oracle_past_the_certificate():
    geo = X.nocert_geometry()
    for label, agg, _, q in X.geometry_queries(geo):
        assert_ref_is_oracle(geo.store, q, agg, f"nocert {label}")


@pytest.mark.parametrize("shape", list(X.THRESHOLD_SHAPES))
def test_reference_equals_oracle_thresholds(shape):
    st = X.threshold_store(shape)
    for K in X.THRESHOLD_K:
        for label, q in X.threshold_queries(shape, K):
            assert_ref_is_oracle(st, q, "max", f"{shape} K {K} {label}")


def test_every_option_set_returns_values():
    """From the oracle alone: in each family, under each rate option set, some query returns values
    (no family's cases are all error outcomes); family b also raises both of its exceptions."""
    seen = {}
    for name, make in X.GEOMETRY_CASES.items():
        geo = make()
        for _, _, o, q in X.geometry_queries(geo):
            seen.setdefault(("a", X.opt_label(o)), set()).add(oracle_outcome(geo.store.batch, q)[1])
    for name, make in X.COUNTER_CASES.items():
        st = make()
        errs = set()
        for _, _, o, q in X.counter_queries(name):
            err = oracle_outcome(st.batch, q)[1]
            errs.add(err)
            seen.setdefault(("b", X.opt_label(o)), set()).add(err)
        assert None in errs, name
    assert {k[1] for k in seen if k[0] == "a"} == {X.opt_label(o) for o in X.A_OPTS}
    assert {k[1] for k in seen if k[0] == "b"} == {X.opt_label(o) for o in X.RATE_OPTS}
    for key, errs in seen.items():
        assert None in errs, key
    b = set().union(*[e for k, e in seen.items() if k[0] == "b"])
    assert b == {None, "IllegalStateException", "RuntimeException"}


# ---- a. the stores hold their edges -----------------------------------------------------------------
def drop_query(geo, fill="none"):
    return X.query(geo.win, "none", "sum", geo.I, fill, dict(counter=True, drop_resets=True))


@pytest.mark.parametrize("name", list(X.GEOMETRY_CASES))
def test_geometry_facts(geos, name):
    geo = geos(name)
    K, hi = geo.K, geo.K - 1
    q = drop_query(geo)
    assert X.slots(geo.win, geo.I) == (geo.B0, K)
    assert (K in X.GEOMETRY_K) or name == "110s"
    # one point a bucket, every span inside the K slots
    for sl, _ in (geo.stream_slots(n, q) for n in geo.names):
        assert sl == sorted(set(sl)) and (not sl or (0 <= sl[0] and sl[-1] <= hi))
    # resets on every listed slot the store has, and on the last
    resets = {s for s in X.RESET_SLOTS + (hi,) if 1 <= s <= hi}
    assert geo.stream_slots("resets", q)[0] == list(range(K))
    assert geo.survivors("resets", q) == [k for k in range(K) if k not in resets]
    assert geo.survivors("resets f32", q) == [k for k in range(K) if k not in resets]
    # first points on slot 63, on slot 64 and on the last slot (a span of one point)
    for n, first in (("first 63", min(63, hi)), ("first 64", min(64, hi)), ("first K-1", hi)):
        assert geo.stream_slots(n, q)[0][0] == first
    assert len(geo.stream_slots("first K-1", q)[0]) == 1 and len(geo.stream_slots("one point", q)[0]) == 1
    # 64 or more resets in a row: a whole chunk without a survivor between two chunks with one
    lo, hi2 = geo.long_reset
    sv = geo.survivors("long reset", q)
    assert [k for k in range(K) if k not in sv] == list(range(lo + 1, hi2 + 1))
    if K >= 129:
        assert hi2 - lo >= 64 and not [k for k in sv if 64 <= k < 128] and [k for k in sv if k < 64] and K > 128
        assert (K <= 129) or [k for k in sv if k >= 128]
    # two points more than 64 slots apart; K >= 129: no item in the chunk between them
    sl = geo.stream_slots("gap", q)[0]
    if K > 66:
        assert len(sl) == 2 and sl[1] - sl[0] > 64
    if K >= 129:
        assert sl[1] // 64 - sl[0] // 64 == 2
    if K > 140:      # (at K = 129 the grid of a fill policy ends before slot 128)
        nan = geo.stream_slots("gap", drop_query(geo, "nan"))
        assert len(nan[0]) >= K - 1 and sum(1 for p in nan[1] if p[2] == p[2]) == 2   # the same gap as NaN buckets
    assert len(geo.stream_slots("two points", q)[0]) == min(2, K)
    # every rate dropped but the second; and a second survivor two chunks after the first
    if K >= 3:
        assert geo.survivors("second only", q) == [1]
        late = geo.survivors("late second", q)
        assert late[:2] == [1, min(hi - 1, 130) + 1]
        if K == 193:
            assert late[1] // 64 == 2
    # the shapes: value classes mixed in one store
    assert {s[2] for s in geo.spans.values()} == {R.LONG, R.F32, R.F64}


def test_one_point_gives_no_output_and_two_points_one(geos):
    geo = geos("K65")
    q = X.query(geo.win, "none", "sum", geo.I, "none", {})
    got = {geo.names[g]: len(ts) for g, ts, _, _ in O.run_query(geo.store.batch, q)}
    assert got["one point"] == 0 and got["first K-1"] == 0 and got["two points"] == 1 and got["resets"] == 64


def test_110s_buckets_do_not_divide_the_hour(geos):
    """The seek drops the point between the scan start and the first boundary, and the grid of a
    fill policy starts one bucket before slot 0 (a fill value that is the first rate's previous
    point and is not handed out itself)."""
    geo = geos("110s")
    assert geo.K == 65 and geo.I == 110000 and 3600000 % geo.I and geo.B0 > R.M0
    i = geo.names.index("gap")
    assert geo.store.series[i][0][0] == R.M0 + 1000 < geo.B0
    q = drop_query(geo)
    assert geo.stream_slots("gap", q)[0][0] == 2          # (the span's own first slot: the early point is in no bucket)
    sl, st = geo.stream_slots("resets", drop_query(geo, "zero"))
    assert sl[0] == -1 and st[0][2] == 0.0 and st[0][0] < X.scan_bounds(q)[0] * 1000
    rates = R.rate_span(st, False, abi.LONG_MAX, 0, False)
    assert rates[1][0] == geo.B0 and rates[1][2] == 1000.0 / 110.0    # against the fill bucket, not (0, 0L)


def test_shapes():
    """One-row series, several one-chunk rows, a walker row (over one chunk of 512 points)."""
    rows = lambda st: [len({t // 3600000 for t, _, _ in s}) for s in st.series]
    per_row = lambda st: max(sum(1 for t, _, _ in s if t // 3600000 == s[0][0] // 3600000) for s in st.series)
    assert set(rows(X.GEOMETRY_CASES["K129"]().store)) == {1}
    assert max(rows(X.GEOMETRY_CASES["K193/3h"]().store)) == 3
    st = X.threshold_store("rows")
    assert set(rows(st)) == {4} and per_row(st) == 360 <= X.CH
    st = X.threshold_store("walker")
    assert set(rows(st)) == {1} and per_row(st) == 1440 > X.CH
    kinds = [{k for _, k, _ in s} for s in X.counter_store().series]
    assert any(len(k) == 3 for k in kinds)       # one span of LONG, F32 and F64 cells


# ---- b. counter arithmetic -----------------------------------------------------------------------------
def test_reset_value_tie_is_exact_in_doubles():
    v0, (eq, up, dn) = X.rate_tie()
    cm, dt = float(X.TIE_MAX), float(X.I_B // 1000)
    assert (cm - v0 + eq) / dt == 1000.0
    assert (cm - v0 + up) / dt == math.nextafter(1000.0, math.inf)
    assert (cm - v0 + dn) / dt == math.nextafter(1000.0, 0.0)
    st = X.counter_store()
    g = list(X.counter_cases()).index("tie")
    q = X.query(X.WIN_B, "none", "sum", X.I_B, "none", dict(counter=True, counter_max=X.TIE_MAX, reset_value=X.TIE_RESET))
    i = [j for j, x in enumerate(st.gids) if x == g][0]
    (_, ts, bits, _) = O.run_query(st.batch, q)[i]
    v = np.asarray(bits).view(np.float64)
    # buckets v0, eq, v0, up, v0, dn, v0, eq: the rates at eq / up / dn (the first rate is consumed)
    assert list(v[[0, 2, 4, 6]]) == [1000.0, 0.0, math.nextafter(1000.0, 0.0), 1000.0]   # strict >: the tie stays
    for rv, want in ((X.TIE_RESET - 1, [0.0, 0.0, 0.0]), (X.TIE_RESET + 1, [1000.0, math.nextafter(1000.0, math.inf), math.nextafter(1000.0, 0.0)])):
        q = X.query(X.WIN_B, "none", "sum", X.I_B, "none", dict(counter=True, counter_max=X.TIE_MAX, reset_value=rv))
        v = np.asarray(O.run_query(st.batch, q)[i][2]).view(np.float64)
        assert list(v[[0, 2, 4]]) == want


def counter_rates(case, opts, fill="none", span=0, fn="sum"):
    st = X.counter_store()
    g = list(X.counter_cases()).index(case)
    i = [j for j, x in enumerate(st.gids) if x == g][span]
    q = X.query(X.WIN_B, "none", fn, X.I_B, fill, opts)
    ss, se = X.scan_bounds(q)
    pts = [(t, k == R.LONG, v) for t, k, v in st.series[i]]
    stream, _ = X.ds_stream(pts, fn, X.I_B, q.ds_fill, ss * 1000, se * 1000)
    return stream, R.rate_span(stream, bool(q.rate_counter), q.rate_counter_max, q.rate_reset_value, bool(q.rate_drop_resets))


def test_counter_facts():
    # a negative first bucket under counter rolls over from (0, 0L)
    stream, rates = counter_rates("negative first", dict(counter=True))
    assert stream[0][2] == -5.0 and rates[0][2] == (float(R.LONG_MAX) - 0.0 + -5.0) / (stream[0][0] / 1000.0) > 0
    # a counter_max below the previous value: the rate stays negative
    stream, rates = counter_rates("above counter_max", dict(counter=True, counter_max=100))
    assert rates[1][2] == (100.0 - 5000.0 + 10.0) / 60.0 < 0
    # the dropped bucket is the previous point of the next rate
    stream, rates = counter_rates("dropped is previous", dict(counter=True, drop_resets=True))
    assert [p[2] for p in stream[:3]] == [10.0, 5.0, 7.0] and [p[0] for p in rates[:2]] == [stream[0][0], stream[2][0]]
    assert rates[1][2] == (7.0 - 5.0) / 60.0
    # differences of +0.0 and -0.0 (a sum bucket is +0.0 + x: last keeps the cell's sign)
    _, rates = counter_rates("zero diffs", {}, fn="last")
    signs = {(r[2], math.copysign(1.0, r[2])) for r in rates if r[2] == 0.0}
    assert signs == {(0.0, 1.0), (0.0, -1.0)}
    # buckets whose cells are all NaN
    stream, _ = counter_rates("nan buckets", {})
    assert sum(1 for p in stream if p[2] != p[2]) == 3
    # FILL_ZERO under counter: the first zero of every gap is a reset (20 -> 0, 25 -> 0, 50 -> 0, 60 -> 0; and 30 -> 25)
    stream, rates = counter_rates("gaps", dict(counter=True, drop_resets=True), "zero")
    assert len(stream) == 60 and len(rates) == 60 - 5
    # the overflowing difference
    for first in ("inf", "gap"):
        st = X.inf_store(first)
        assert oracle_outcome(st.batch, X.query(X.WIN_B, "sum", "sum", X.I_B, "none", {}))[1] == "IllegalStateException"
        assert oracle_outcome(st.batch, X.query(X.WIN_B, "count", "sum", X.I_B, "none", {}))[1] is None
        want = "IllegalStateException" if first == "inf" else "RuntimeException"
        assert oracle_outcome(st.batch, X.query(X.WIN_B, "sum", "sum", X.I_B, "scalar", {}))[1] == want   # the first group's error
        assert oracle_outcome(st.batch, X.query(X.WIN_B, "sum", "sum", X.I_B, "scalar"))[1] == "RuntimeException"   # (no rate: no infinity)
    assert oracle_outcome(X.full_store().batch, X.query(X.WIN_B, "sum", "sum", X.I_B, "scalar", {}))[1] is None


# ---- c. the thresholds ------------------------------------------------------------------------------------
def test_thresholds_come_from_the_kernels_formulas():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opentsdb_amd", "csrc")
    text = open(os.path.join(src, "kcommon.h")).read() + open(os.path.join(src, "engine.h")).read()
    assert int(re.search(r"constexpr int VBUF = (\d+);", text).group(1)) == X.VBUF
    assert int(re.search(r"constexpr int CH_ROWS = (\d+);", text).group(1)) == X.CH
    assert re.search(r"constexpr int CH = CH_ROWS;", text)
    assert X.fast_wave_lds(X.K_FUSED_RATE, True) <= 32768 < X.fast_wave_lds(X.K_FUSED_RATE + 1, True)
    assert X.fast_wave_lds(X.K_FUSED, False) <= 32768 < X.fast_wave_lds(X.K_FUSED + 1, False)
    assert X.grid_wave_lds(X.K_GRID_LDS, True) <= 40960 < X.grid_wave_lds(X.K_GRID_LDS + 1, True)
    # between the two fused-pass bounds only the rate query takes the dense split
    assert X.K_FUSED_RATE < X.K_GRID_LDS < X.K_GRID_LDS + 1 < X.K_FUSED < X.K_DAY
    for K in X.THRESHOLD_K:
        for shape in X.THRESHOLD_SHAPES:
            q = X.threshold_queries(shape, K)[0][1]
            assert X.slots(X.threshold_window(shape), q.ds_interval_ms)[1] == K
