"""GPU parity of the rate over downsampled buckets (the rate branch of emit_series_to,
csrc/kcommon.h) at the 64-lane chunk boundaries, at the edges of the counter arithmetic and on both
sides of the K thresholds of its routes, against the CPU oracle: the same groups, timestamps and
Java exception, the same bits under none / max / min / count / p50 / p99, the project's REL_TOL
under sum / avg and DEV_TOL under dev.  tests/test_rate_edges_cpu.py shows without a GPU that the
stores of tests/rate_edges.py hold their edges and that a plain Python restatement of the query
equals the oracle on every case used here.

a, b: every query through k_grid (FAST = 0) and through each downsample path's switch; each path
      equals the oracle and equals k_grid bit for bit (HWIN = 1 / 2: hwin_slots refuses a rate
      query, the result must not change).
c:    the default path and FAST = 0 at the K on both sides of the fused pass's LDS bound (with and
      without rate), of k_grid's slots-in-LDS bound and at a day of 1m buckets, with the route
      shown by eng.timing().
Then the other consumers of the emitter (percentile downsampling, the percentile group-by, the
ordered fold, run_multi, the rollup read path, calendar months, 0all), the resident batch
(append, trim) and a sharded run.
"""
from __future__ import annotations

import numpy as np
import pytest

from opentsdb_amd import abi
from opentsdb_amd import engine as E
from opentsdb_amd.engine import options
from oracle import oracle as O
from tests import append_util as AU
from tests import index_ref as IR
from tests import rate_edges as X
from tests import raw_edges as R
from tests import value_edges as V
from tests.test_gpu_parity import DEV_TOL, REL_TOL
from tests.test_gpu_value_edges import assert_same, check_paths, engine_outcome, oracle_outcome
from tests.trim_util import trim_batch

pytestmark = pytest.mark.gpu

PATHS = [("default", {}), ("SHORT=0", dict(SHORT=0)), ("ROWS=0", dict(ROWS=0)), ("REGULAR=0", dict(REGULAR=0)),
         ("HWIN=1", dict(HWIN=1)), ("HWIN=2", dict(HWIN=2))]
SEQ_PATHS = [("default", {}), ("SEQ=0", dict(SEQ=0)), ("SEQ_ROWS=0", dict(SEQ_ROWS=0)), ("SEQ_WAVE=0", dict(SEQ_WAVE=0))]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def cmp_of(agg):
    return X.compare(agg, REL_TOL, DEV_TOL)


# ---- a. chunk geometry ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.GEOMETRY_CASES))
def test_chunk_geometry(eng, name):
    geo = X.GEOMETRY_CASES[name]()
    eng.load(geo.store.batch)
    for label, agg, _, q in X.geometry_queries(geo):
        check_paths(eng, geo.store, q, f"{name} {label}", paths=PATHS, cmp=cmp_of(agg))


def test_chunk_geometry_past_the_certificate(eng):
    """The K = 129 store in values past the exactness certificate (every row ROW_NOCERT): the
    sequential dense kernels and, without them, k_grid."""
    geo = X.nocert_geometry()
    eng.load(geo.store.batch)
    _, flags, _, _ = eng.debug_rows()
    assert (flags & IR.ROW_NOCERT).all()
    for label, agg, _, q in X.geometry_queries(geo):
        check_paths(eng, geo.store, q, f"nocert {label}", paths=SEQ_PATHS, cmp=cmp_of(agg))


# ---- b. counter arithmetic --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.COUNTER_CASES))
def test_counter_arithmetic(eng, name):
    st = X.COUNTER_CASES[name]()
    eng.load(st.batch)
    for label, agg, _, q in X.counter_queries(name):
        check_paths(eng, st, q, f"{name} {label}", paths=PATHS, cmp=cmp_of(agg))


@pytest.mark.parametrize("first", ["inf", "gap"])
def test_fill_scalar_error_precedence(eng, first):
    """FILL_SCALAR with a group that raises IllegalStateException (an infinite rate) and a group
    that raises RuntimeException (a missing bucket): the exception of the group that comes first.

    The device error word keeps the first code any kernel sets and carries no group; tsdbhip_run
    settles the order on its error path (scalar_fill_error, csrc/engine.cpp), whichever kernels ran."""
    st = X.inf_store(first)
    eng.load(st.batch)
    bad = []
    for label, agg, q in X.precedence_queries():
        want = oracle_outcome(st.batch, q)
        for name, opts in [("FAST=0", dict(FAST=0))] + PATHS:
            got = engine_outcome(eng, q, **opts)
            if got[1] != want[1]:
                bad.append(f"{label} [{name}]: engine {got[1]}, oracle {want[1]}")
            elif want[1] is None:
                cmp_of(agg)(got[0], want[0], f"{first} first {label} [{name}]")
    print(f"measured {first} first: {len(bad)} of {7 * len(X.precedence_queries())} runs raise another exception")
    assert not bad, bad


def test_leading_fill_bucket_under_scalar_fill(eng):
    """Every slot holds a point, the bucket FillingDownsampler puts before slot 0 does not: under
    FILL_SCALAR the rate query raises RuntimeException, under ZERO and NAN that bucket is the first
    rate's previous point."""
    st = X.lead_store()
    eng.load(st.batch)
    for label, agg, q in X.lead_queries():
        check_paths(eng, st, q, f"lead {label}", paths=PATHS, cmp=cmp_of(agg))


# ---- c. the K thresholds ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def threshold_stores():
    return {shape: X.threshold_store(shape) for shape in X.THRESHOLD_SHAPES}


@pytest.mark.parametrize("K", X.THRESHOLD_K)
@pytest.mark.parametrize("shape", list(X.THRESHOLD_SHAPES))
def test_route_thresholds(eng, threshold_stores, shape, K):
    """The streaming routes (the fused pass up to K_FUSED_RATE with rate and K_FUSED without, the
    dense split with k_emit over the HBM buckets above) answer the default path: fast_ms > 0 and no
    tile handed back; under FAST = 0 k_grid answers (fast_ms == 0), with its slots in LDS up to
    K_GRID_LDS with rate and in HBM above.  Every result equals the oracle and k_grid."""
    st = threshold_stores[shape]
    eng.load(st.batch)
    for label, q in X.threshold_queries(shape, K):
        ctx = f"{shape} K {K} {label}"
        want = oracle_outcome(st.batch, q)
        assert want[1] is None
        agg = abi.AGGREGATOR_NAMES[q.aggregator]
        fast, grid = engine_outcome(eng, q), engine_outcome(eng, q, FAST=0)
        assert_same(fast, want, f"{ctx} [default]", cmp_of(agg))
        assert_same(grid, want, f"{ctx} [FAST=0]", cmp_of(agg))
        V.assert_bits(fast[0], grid[0], f"{ctx} [default] against k_grid")
        assert fast[2].fast_ms > 0 and fast[2].redo_tiles == 0, f"{ctx}: no streaming pass answered"
        assert grid[2].fast_ms == 0, f"{ctx}: a streaming pass ran under FAST=0"


# ---- the other consumers of the emitter ----------------------------------------------------------------------
CONSUMER_CASES = ["K65", "K129"]
CONSUMER_OPTS = [X.A_OPTS[0], X.A_OPTS[2], X.A_OPTS[3]]


@pytest.fixture(scope="module")
def consumer_geo():
    return {name: X.GEOMETRY_CASES[name]() for name in CONSUMER_CASES}


def check_variants(eng, store, q, ctx, variants, cmp=V.assert_bits):
    want = oracle_outcome(store.batch, q)
    first = None
    for name, opts in variants:
        got = engine_outcome(eng, q, **opts)
        assert_same(got, want, f"{ctx} [{name}]", cmp)
        if want[1] is None:
            if first is None:
                first = got
            else:
                V.assert_bits(got[0], first[0], f"{ctx} [{name}] against [{variants[0][0]}]")
    return want


@pytest.mark.parametrize("name", CONSUMER_CASES)
def test_percentile_downsampling_with_rate(eng, consumer_geo, name):
    geo = consumer_geo[name]
    eng.load(geo.store.batch)
    for fn in ("p99", "median"):
        for fill in ("none", "zero"):
            for o in CONSUMER_OPTS:
                for agg in ("none", "max", "sum"):
                    q = X.query(geo.win, agg, fn, geo.I, fill, o)
                    check_variants(eng, geo.store, q, f"{name} {agg}:{fn} fill {fill} {X.opt_label(o)}",
                                   [("default", {}), ("FAST=0", dict(FAST=0)), ("PCT_ROWS=0", dict(PCT_ROWS=0))], cmp_of(agg))


SEL_GROUP = [("default", {}), ("SEL_FUSED=0", dict(SEL_FUSED=0)), ("SEL_COLS=0", dict(SEL_COLS=0)),
             ("SEL_WIN=0", dict(SEL_WIN=0)), ("SEL_WIN=2", dict(SEL_WIN=2))]


@pytest.mark.parametrize("name", CONSUMER_CASES)
def test_percentile_group_by_with_rate(eng, consumer_geo, name):
    geo = consumer_geo[name]
    eng.load(geo.store.batch)
    for agg in ("p50", "p99"):
        for fill in ("none", "nan", "zero"):
            for o in CONSUMER_OPTS:
                q = X.query(geo.win, agg, "sum", geo.I, fill, o)
                check_variants(eng, geo.store, q, f"{name} {agg}:sum fill {fill} {X.opt_label(o)}", SEL_GROUP)


@pytest.mark.parametrize("name", CONSUMER_CASES)
def test_ordered_fold_with_rate(eng, consumer_geo, name):
    """QF_ORDERED: the group's spans in SpanGroup order, the oracle's bits."""
    geo = consumer_geo[name]
    eng.load(geo.store.batch)
    for agg in ("sum", "avg", "dev"):
        for fill in ("none", "nan", "zero"):
            for o in CONSUMER_OPTS:
                q = X.query(geo.win, agg, "sum", geo.I, fill, o)
                q.flags = abi.QF_ORDERED
                assert_same(engine_outcome(eng, q), oracle_outcome(geo.store.batch, q),
                            f"{name} ordered {agg} fill {fill} {X.opt_label(o)}")


@pytest.mark.parametrize("name", CONSUMER_CASES)
def test_run_multi_with_rate(eng, consumer_geo, name):
    """run_multi of a rate query, its twin without rate and a rate query with other options (the
    fused pass has no rate variant: the call falls back): each result has the single query's bits."""
    geo = consumer_geo[name]
    eng.load(geo.store.batch)
    for agg in ("max", "sum", "count"):
        qs = [X.query(geo.win, agg, "sum", geo.I, "none", dict(counter=True, drop_resets=True)),
              X.query(geo.win, agg, "sum", geo.I),
              X.query(geo.win, agg, "sum", geo.I, "none", dict(counter=True, counter_max=1 << 32, reset_value=1000))]
        single = [eng.run(q) for q in qs]
        for q, s in zip(qs, single):
            cmp_of(agg)(s, O.run_query(geo.store.batch, q), f"{name} {agg} single")
        for fuse in (1, 0):
            with options(MULTI_FUSE=fuse):
                got = eng.run_multi(qs)
            assert len(got) == len(qs)
            for i, (g, s) in enumerate(zip(got, single)):
                V.assert_bits(g, s, f"{name} {agg} run_multi query {i} MULTI_FUSE={fuse}")


def test_rollup_read_with_rate(eng):
    """The rollup read path with rate over a day of 10m cells (K = 144) and three days of 30m
    buckets, cells missing at random: counter options, bit for bit under none / max (a count
    group-by of a rollup query sums the rolled-up counts: TsdbQuery turns it into sum)."""
    from tests.test_gpu_rollup_read import B, _q, random_table
    rng = np.random.default_rng(7)
    rb = random_table(rng, 8, 2, 3, p_sum=0.85, p_cnt=0.85)
    eng.load_rollup(rb)
    for ds in ("10m-sum", "30m-max", "10m-sum-zero", "10m-avg-nan"):
        for o in CONSUMER_OPTS:
            for agg in ("none", "max", "count", "sum"):
                q = _q(ds, agg, start=B + 1800, end=B + 86400 + (2 * 86400 if ds.startswith("30m") else 0))
                q.rate, q.rate_counter, q.rate_drop_resets = 1, int(o.get("counter", False)), int(o.get("drop_resets", False))
                q.rate_counter_max, q.rate_reset_value = o.get("counter_max", abi.LONG_MAX), o.get("reset_value", 0)
                try:
                    want = O.run_rollup_query(rb, q), None
                except O.OracleError as e:
                    want = None, e.java
                for name, opts in (("default", {}), ("RO_FUSE=0", dict(RO_FUSE=0))):
                    assert_same(engine_outcome(eng, q, **opts), want, f"rollup {ds} {agg} {X.opt_label(o)} [{name}]",
                                cmp_of("sum" if agg == "count" else agg))


def spec_query(spec, win, agg, o):
    q = abi.new_query(win[0], win[1], agg, rate=True, **o)
    p = O.parse_downsample(spec)
    for f in ("ds_function", "ds_fill", "ds_all", "ds_calendar", "ds_interval_ms"):
        setattr(q, f, getattr(p, f))
    return q


def month_store() -> R.RStore:
    """Three counters (two groups) with a point every 53 h over 200 days: calendar months hold 13 to
    15 points, and the time between two buckets differs from month to month."""
    ts = [R.M0 + 53 * 3600 * 1000 * i + 7000 for i in range(90)]
    series = []
    for s, kind in enumerate((R.LONG, R.F64, R.LONG)):
        v, vals = 100 * s, []
        for i in range(90):
            v = 3 + s if (i + 5 * s) % 31 == 30 else v + 2 + (i * (s + 2)) % 7
            vals.append(v if kind == R.LONG else 0.5 * v)
        series.append(R.span(ts, vals, kind))
    return R.RStore(series, [0, 0, 1])


def test_calendar_months_and_all_with_rate(eng):
    """1nc buckets (dt differs from bucket to bucket) and 0all with rate: the oracle's outcome,
    whatever it is, on the default path and through k_grid."""
    st = month_store()
    eng.load(st.batch)
    win = (R.T0, R.T0 + 200 * 86400)
    outcomes = set()
    for spec in ("1nc-sum", "1nc-max-zero", "1nc-last-nan", "0all-sum", "0all-max"):
        for o in X.A_OPTS:
            for agg in ("none", "max", "sum", "count"):
                q = spec_query(spec, win, agg, o)
                want = oracle_outcome(st.batch, q)
                outcomes.add((spec[:4], want[1]))
                for name, opts in (("default", {}), ("FAST=0", dict(FAST=0))):
                    assert_same(engine_outcome(eng, q, **opts), want, f"{spec} {agg} {X.opt_label(o)} [{name}]", cmp_of(agg))
    assert ("1nc-", None) in outcomes


# ---- the resident batch -----------------------------------------------------------------------------------------
def test_append_and_trim_move_the_first_rate(eng):
    """Load an hour, append the next one (its first bucket is a reset), then trim the first: after
    each step the rate query (counter, drop_resets) equals the one on a fresh load of the same rows
    bit for bit -- and the first surviving rate changes when its previous point is evicted."""
    H = R.H
    ts = np.arange(R.T0, R.T0 + 2 * H, 20, dtype=np.int64)
    points, gids = [], [0, 0, 1, 1]
    for s in range(4):
        v = 1000 * (s + 1) + 5 * np.arange(len(ts)) + (np.arange(len(ts)) * (s + 3)) % 7
        v[len(ts) // 2:] -= v[len(ts) // 2] - (s + 1)          # hour 2 starts again at s + 1: a reset
        v[len(ts) // 2 + 70:] -= 40 * (s + 1)                  # and a later one, on slot 70 of the hour
        points.append(AU.Points(ts * 1000, lvals=v))
    A, D, idx, new, full = AU.split(points, gids, R.T0 + H)
    trimmed = trim_batch(full, R.T0 + H)
    qs = [X.query((R.T0 + 200, R.T0 + 2 * H - 200), agg, "sum", 20000, fill, dict(counter=True, drop_resets=True))
          for agg in ("none", "max", "sum") for fill in ("none", "zero")]
    fresh = {}
    for key, b in (("loaded", A), ("appended", full), ("trimmed", trimmed)):
        eng.load(b)
        fresh[key] = [eng.run(q) for q in qs]
        for q, g in zip(qs, fresh[key]):
            cmp_of(abi.AGGREGATOR_NAMES[q.aggregator])(g, O.run_query(b, q), f"fresh {key}")

    def check(key):
        for i, (q, w) in enumerate(zip(qs, fresh[key])):
            V.assert_bits(eng.run(q), w, f"{key} query {i} against a fresh load")

    eng.load(A)
    check("loaded")
    eng.append(D, idx, new)
    check("appended")
    eng.trim(R.T0 + H)
    check("trimmed")
    # hour 2's first bucket under zero fill (query 1: none, one result a series): a reset after the
    # append, dropped; after the trim the buckets before it are fill zeros and its rate survives
    at = (R.T0 + H) * 1000
    assert all(at not in g[1] for g in fresh["appended"][1]) and all(at in g[1] for g in fresh["trimmed"][1])


# ---- sharding -------------------------------------------------------------------------------------------------
def test_sharded_run_equals_one_engine(eng):
    from tests.test_gpu_dist import run_sharded
    geo = X.GEOMETRY_CASES["K129"]()
    engines = [E.Engine(0), E.Engine(0)]
    try:
        eng.load(geo.store.batch)
        for agg in ("max", "min", "count", "sum"):
            for fill in ("none", "zero"):
                for o in CONSUMER_OPTS:
                    q = X.query(geo.win, agg, "sum", geo.I, fill, o)
                    one = eng.run(q)
                    ctx = f"sharded {agg} fill {fill} {X.opt_label(o)}"
                    cmp_of(agg)(one, O.run_query(geo.store.batch, q), ctx + " one engine")
                    cmp_of(agg)(run_sharded(engines, geo.store.batch, q, 2), one, ctx)
    finally:
        for e in engines:
            e.close()
