"""GPU parity of rollup generation on every kernel route and bucket geometry: the stores of
tests/rollup_paths.py (proved on the host by tests/test_rollup_paths_cpu.py) against
oracle/rollup.generate, byte for byte, with the route asserted from Engine.debug_rollup() --
(streaming pass launched, series it ran over, series class A handed back, series k_rollup_agg
reduced) -- and every case repeated under option FAST = 0, where k_rollup_agg reduces every
series.

The streaming pass runs while K <= 1170, and K covers the whole hour rows the window's scan
touches: under 1s, 2s and 3s cells (3600, 1800, 1200 slots an hour) it never runs, under 5s
only for a window inside one hour row.  Those cases therefore pin k_rollup_agg (route
"general"); the streaming pass's per-datapoint fold and its split vote are pinned by the short
windows of case a and by the 8 s vle rows under 7s, 13s and 45s cells."""
from __future__ import annotations

import pytest

from oracle import rollup as R
from tests import rollup_paths as P

pytestmark = pytest.mark.gpu

T0, START, END, WIN0, H1, H2 = P.T0, P.START, P.END, P.WIN0, P.H1, P.H2
FUNCS = P.FUNCS
GENERAL = "general"


@pytest.fixture(scope="module")
def eng():
    from opentsdb_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def oracle_outcome(store, interval, span, start, end, funcs):
    try:
        return R.generate(store, R.Interval(interval, span), start, end, funcs), None
    except R.RollupError:
        return None, "IllegalArgumentException"


def engine_outcome(eng, interval, span, start, end, funcs):
    from opentsdb_amd import engine
    try:
        cells = eng.rollup(engine.rollup_interval(interval, span), start, end, funcs)
    except engine.EngineError as e:
        return None, e.java
    return [cells.cell(i) for i in range(len(cells))], None


def same_cells(got, exp, ctx):
    assert len(got) == len(exp), (ctx, len(got), len(exp))
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g == e, (ctx, i, g, e)


def check(eng, store, interval, span, start, end, funcs, route):
    """The engine's cells are the oracle's byte for byte (or both refuse with an
    IllegalArgumentException), the run took `route` -- GENERAL, or (series class A handed back,
    series k_rollup_agg reduced) of a streaming run --, and FAST = 0 gives the same cells."""
    from opentsdb_amd import engine
    I = P.interval_seconds(interval)
    n, not_a, neither, _A, _B = P.route_bounds(store, I, start, end)
    if route == GENERAL:
        want_route = (0, 0, 0, n)
    else:
        assert P.streams(I, start, end), "the case names a streaming route for a window beyond the LDS limit"
        assert route[0] >= not_a and route[1] >= neither and route[0] >= route[1], (route, not_a, neither)
        want_route = (1, n) + tuple(route)
    exp, exp_err = oracle_outcome(store, interval, span, start, end, funcs)
    eng.load(store)
    got, got_err = engine_outcome(eng, interval, span, start, end, funcs)
    got_route = eng.debug_rollup()
    with engine.options(FAST=0):
        got0, got0_err = engine_outcome(eng, interval, span, start, end, funcs)
        route0 = eng.debug_rollup()
    print(f"{interval}/{span} [{start - T0}, {end - T0}): route {got_route}, FAST=0 {route0}, "
          f"cells {None if exp is None else len(exp)}, oracle {exp_err}, engine {got_err} / {got0_err}")
    assert got_err == exp_err and got0_err == exp_err
    assert got_route == want_route, (got_route, want_route)
    assert route0 == (0, 0, 0, n)
    if exp is not None:
        same_cells(got, exp, "streaming" if want_route[0] else "general")
        same_cells(got0, exp, "FAST=0")
    return exp


# ---- a / b: certified classes x intervals ----------------------------------------------------
# the route each interval's window takes (tests/test_rollup_paths_cpu.py test_case_a_window_side)
A_STREAMS = {"1s": False, "2s": False, "3s": False, "5s": False, "7s": True, "13s": True, "45s": True, "90s": True,
             "1m": True, "5m": True, "1h": True}


@pytest.mark.parametrize("interval,span", P.A_INTERVALS)
@pytest.mark.parametrize("name", P.CERTIFIED)
def test_a_certified_classes(eng, name, interval, span):
    store = P.uniform(name)
    start, end = P.a_window(interval)
    n = len(store.series_row_ptr) - 1
    if not A_STREAMS[interval]:
        route = GENERAL
    elif name == "vle7s":
        route = (n, n)     # 514 points in the full row: k_rollup_fast<2, 0> hands every series back
    else:
        route = (0, 0)
    exp = check(eng, store, interval, span, start, end, FUNCS, route)
    assert exp is None or len(exp) > 0


@pytest.mark.parametrize("interval,span,win", P.A_SHORT)
@pytest.mark.parametrize("name", ["q2f32", "q2f64", "q4f32", "q4f64", "vle8s"])
def test_a_short_window_streams_small_cells(eng, name, interval, span, win):
    """Inside one hour row the pass runs under 4s, 5s and 6s cells: on 1 s data 5s splits the
    vote (lanes of two and of three runs), 4s and 6s put a bucket change in every lane; on
    500 ms data every lane has one or two runs, on 8 s data each datapoint its own bucket.  13s
    (refused over case a's window, by the oracle and the engine alike) gives its cells here."""
    exp = check(eng, P.uniform(name), interval, span, *win, FUNCS, (0, 0))
    assert exp


def test_b_general_kernel_whole_store_1s(eng):
    """1s/1h over all three rows, K = 10800: no streaming pass at all."""
    for name in ("q2f32", "vle8s"):
        exp = check(eng, P.uniform(name), "1s", "1h", START, END, FUNCS, GENERAL)
        assert exp


# ---- c: uncertified series --------------------------------------------------------------------
@pytest.mark.parametrize("interval,span", P.C_INTERVALS)
@pytest.mark.parametrize("name", P.UNCERTIFIED)
def test_c_uncertified(eng, name, interval, span):
    """Full-mantissa doubles: the streaming pass (where K allows it) folds every series to its
    end, fails the certificate there and hands all of them back; k_rollup_agg then takes its
    sequential loop.  Once inside the second row (K small), once from the start of the day over the three rows."""
    store = P.uniform(name)
    n = len(store.series_row_ptr) - 1
    for start, end in P.C_WINDOWS:
        route = (n, n) if P.streams(P.interval_seconds(interval), start, end) else GENERAL
        exp = check(eng, store, interval, span, start, end, FUNCS, route)
    assert exp   # (the second window holds the start of the day: every interval has a cell)


# ---- d: the class A -> class B -> general chain -------------------------------------------------
@pytest.mark.parametrize("interval,span,start", [("1m", "1h", START), ("7s", "1h", WIN0), ("1h", "1d", START)])
def test_d_chain(eng, interval, span, start):
    store = P.chain()
    names = [n for n, _ in P.CHAIN_SERIES]
    # 13 grouped series; class A finishes the four float32 ones, class B the three vle ones; the
    # general kernel gets the two 4-byte/float64 series, the full-mantissa one and the three late
    # breakers, whose first rows class A had already folded
    exp = check(eng, store, interval, span, start, END, FUNCS, (13 - 4, 13 - 4 - 3))
    if exp is not None:
        ser = [c[0] for c in exp]
        assert names.index("nogroup") not in ser
        for late in P.CHAIN_LATE:
            assert names.index(late) in ser
        per_fn = len(ser) // 4
        assert all(a <= b for a, b in zip(ser[:per_fn], ser[1:per_fn]))      # batch series order


# ---- e: window edges ---------------------------------------------------------------------------
EDGES = {
    "end_30s_into_a_bucket": (H1 + 540, H1 + 630, 12),
    "start_30s_into_a_bucket": (H1 + 570, H1 + 900, 30),
    "inside_one_lane": (H1 + 58, H1 + 62, 6),
    "before_the_data": (T0 - 7200, T0 - 3600, 0),
    "after_the_data": (END + 7200, END + 10800, 0),
    "wider_than_the_data": (T0 - 86400, T0 + 86400, None),
    "first_point_to_one_past_the_last": (START, END, None),
}


@pytest.mark.parametrize("edge", list(EDGES))
@pytest.mark.parametrize("name", ["q2f32", "fm1s"])
def test_e_window_edges(eng, name, edge):
    start, end, n_sum = EDGES[edge]
    store = P.uniform(name)
    n = 6
    if not P.streams(60, start, end):
        route = GENERAL
    elif name == "fm1s" and edge not in ("before_the_data", "after_the_data"):
        route = (n, n)
    else:
        route = (0, 0)      # (a series without a row in the scan range finishes with no cell)
    assert (route == GENERAL) == (edge == "wider_than_the_data")
    exp = check(eng, store, "1m", "1h", start, end, FUNCS, route)
    if n_sum is not None:
        assert len(exp) == 4 * n_sum
    else:
        assert len(exp) >= 4 * n * 70


# ---- f: NaN values -----------------------------------------------------------------------------
def test_f_nan_counts_3s(eng):
    exp = check(eng, P.nans(), "3s", "1h", START, END, (("count", 1),), GENERAL)
    zeros = sum(1 for c in exp if c[3] == b"\x00")
    assert zeros >= 1200 and any(c[3] == b"\x01" for c in exp)     # series 2's all-NaN row, and more


def test_f_nan_all_functions_1m(eng):
    # series 0 and 1 stream; the six with NaN rows are handed back, and no second class exists
    exp = check(eng, P.nans(), "1m", "1h", H2, END, FUNCS, (6, 6))
    counts = [c for c in exp if c[2][0] == 1]
    assert any(0 < c[3][0] < 20 for c in counts) and any(c[3] == b"\x14" for c in counts)   # 20 points a minute


def test_f_nan_sum_3s_rejected(eng):
    exp = check(eng, P.nans(), "3s", "1h", START, END, (("sum", 0),), GENERAL)
    assert exp is None
    exp = check(eng, P.nans(), "1m", "1h", START, END, (("max", 2),), (6, 6))    # series 2's all-NaN hour
    assert exp is None


# ---- g: rows stored out of time order ------------------------------------------------------------
@pytest.mark.parametrize("interval,span", [("1m", "1h"), ("7s", "1h"), ("10m", "1d")])
@pytest.mark.parametrize("name", ["swap_dup", "ms"])
def test_g_stored_order(eng, name, interval, span):
    """Every series has a row that is out of order or of mixed kinds: the streaming pass hands
    all 30 back, and k_rollup_agg applies the stored-order rule (so_apply)."""
    check(eng, P.stored_order(name), interval, span, T0 + 600, T0 + 6600, FUNCS, (30, 30))


# ---- h: points around bucket boundaries -----------------------------------------------------------
@pytest.mark.parametrize("interval,span", [("7s", "2h"), ("45s", "1h")])
def test_h_boundary(eng, interval, span):
    exp = check(eng, P.boundary(), interval, span, *P.BOUNDARY_WINDOW, FUNCS, (0, 0))
    if exp is not None:
        # the series on this interval's boundaries: three points a bucket
        s = 0 if interval == "7s" else 3
        counts = [c[3] for c in exp if c[2][0] == 1 and c[0] == s]
        assert counts and set(counts[1:-1]) == {b"\x03"}


# ---- i: two repeated devices -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["groups", "series"])
def test_i_two_devices(eng, mode):
    from opentsdb_amd import engine
    cases = [(P.chain(), "1m", "1h", START, END), (P.uniform("q4f32"), "45s", "1h", *P.a_window("45s"))]
    md = engine.Engine(devices=[0, 0])
    try:
        md.shard_mode(engine.SHARD_GROUPS if mode == "groups" else engine.SHARD_SERIES)
        for store, interval, span, start, end in cases:
            exp, err = oracle_outcome(store, interval, span, start, end, FUNCS)
            assert err is None
            eng.load(store)
            one, _ = engine_outcome(eng, interval, span, start, end, FUNCS)
            md.load(store)
            got, got_err = engine_outcome(md, interval, span, start, end, FUNCS)
            assert got_err is None
            same_cells(got, one, f"two devices, {mode} shards")
            same_cells(got, exp, "oracle")
        with pytest.raises(engine.EngineError) as ei:
            md.debug_rollup()
        assert ei.value.java == "NotImplemented"
    finally:
        md.close()


def test_debug_rollup_before_any_run():
    from opentsdb_amd.engine import Engine
    e = Engine(0)
    try:
        assert e.debug_rollup() == (0, 0, 0, 0)
    finally:
        e.close()
