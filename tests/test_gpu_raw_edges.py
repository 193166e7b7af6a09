"""GPU parity of the raw path and of the group-by LERP at the value edges, against the CPU oracle
bit for bit (value_edges.assert_bits: the sign of zero included, a NaN matches a NaN), the Java
exception's name where the oracle raises.  tests/test_raw_edges_cpu.py shows without a GPU that
the stores of tests/raw_edges.py are what they claim to be and that a plain Python restatement of
the raw path equals the oracle on every query used here.

A. k_raw_eval / k_raw_rate: the guards of the strip-wide long LERP (lerpw_*) and the general
   path beside it (option RAW_LERPW = 0), the limits of jdiv_pos and wrapped products, NaN,
   infinities, signed zeros, subnormals and overflowing double LERPs in float64 and float32
   cells, longs above 2^53 in a float group, the float flag of a span not yet started, rate /
   counter edges, and unions of 1 .. 1025 points with spans at the chunk boundaries.
B. the raw percentile kernels (k_raw_top, k_raw_vals, k_raw_sel*; options RAW_SEL_TOP = 0 and
   RAW_SEL_REG = 0) over the same stores, and a double LERP that overflows to +Inf while ~300
   operands are present: k_raw_top may prune a span only when its LERP cannot overflow.
C. the group-by of the downsampled path over missing buckets (interp / slot_contribution, the
   fused multi-aggregator pass, k_emit) in the value_edges stores, through every path's switch.

Not covered here: windows of 2^32 - 1 and 2^32 ms (49.7 days of hour rows); that guard of
lerpw_init is left to the CPU arithmetic tests (tests/test_raw_edges_cpu.py,
tests/test_lerp_window_math.py).
"""
from __future__ import annotations

import pytest

from opentsdb_amd import abi
from opentsdb_amd import engine as E
from opentsdb_amd.engine import EngineError, options
from tests import raw_edges as R
from tests import value_edges as V
from tests.test_gpu_value_edges import assert_same, check_paths, engine_outcome, oracle_outcome, query

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def check_variants(eng, store, q, ctx, variants):
    """The resident store's query under every option set of `variants`: each equals the oracle
    (bits, or the exception's name), and all equal one another."""
    want = oracle_outcome(store.batch, q)
    first = None
    for name, opts in variants:
        got = engine_outcome(eng, q, **opts)
        assert_same(got, want, f"{ctx} [{name}]")
        if want[1] is None:
            if first is None:
                first = got
            else:
                V.assert_bits(got[0], first[0], f"{ctx} [{name}] against [{variants[0][0]}]")
    return want


# ---- A. k_raw_eval, k_raw_rate -----------------------------------------------------------------------
LERPW = [("default", {}), ("RAW_LERPW=0", dict(RAW_LERPW=0))]


@pytest.mark.parametrize("name", list(R.RAW_CASES))
def test_raw_eval_edges(eng, name):
    st = R.RAW_CASES[name][0]()
    eng.load(st.batch)
    for label, q in R.queries_of(name):
        check_variants(eng, st, q, f"{name} {label}", LERPW)


# ---- B. raw percentiles ----------------------------------------------------------------------------------
SEL = [("default", {}), ("RAW_SEL_TOP=0", dict(RAW_SEL_TOP=0)), ("RAW_SEL_REG=0", dict(RAW_SEL_REG=0))]


@pytest.mark.parametrize("name", [n for n in R.PCT_CASES if not n.startswith("pct_overflow")])
def test_raw_percentile_edges(eng, name):
    st = R.PCT_CASES[name][0]()
    eng.load(st.batch)
    for label, q in R.pct_queries_of(name):
        check_variants(eng, st, q, f"{name} {label}", SEL)


@pytest.mark.parametrize("sign", ["+", "-"])
def test_raw_percentile_of_an_overflowing_lerp(eng, sign):
    """Span A runs from 0.0 to +-1e305 beside 299 spans of +-1e306: (x - x0) (y1 - y0) overflows, so
    Java's operand of A is +-Inf although both ends are small.  +: the infinity is the largest
    operand; p99 lies between two finite keys below it (a kernel that takes A's operand to lie
    within [y0, y1] and prunes it shifts every rank by one), p999 is the infinity itself and the
    oracle raises.  -: the infinity is the smallest operand and leaving it out of the top keys is
    right."""
    st = R.PCT_CASES[f"pct_overflow/{sign}"][0]()
    eng.load(st.batch)
    outcomes = set()
    for label, q in R.pct_queries_of(f"pct_overflow/{sign}"):
        outcomes.add((label, check_variants(eng, st, q, f"pct_overflow/{sign} {label}", SEL)[1]))
    if sign == "+":
        assert ("p99", None) in outcomes and ("p999", "IllegalStateException") in outcomes
    else:
        assert {e for _, e in outcomes} == {None}


# ---- C. group-by LERP over missing buckets ---------------------------------------------------------------
SPARSE = R.sparse_stores()
SPARSE_PATHS = [("default", {}), ("SHORT=0", dict(SHORT=0)), ("ROWS=0", dict(ROWS=0)), ("HWIN=0", dict(HWIN=0)),
                ("HWIN=1", dict(HWIN=1))]
GROUP_AGGS = ["sum", "min", "max", "avg", "count", "first", "last", "mimmin", "mimmax", "zimsum"]
DS_FUNS = ["sum", "min", "first"]
INTERVAL = 60000


@pytest.fixture(scope="module")
def sparse_store():
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()          # (one store at a time)
            cache[name] = SPARSE[name][0]()
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(SPARSE))
def test_group_by_lerp_over_missing_buckets(eng, sparse_store, name):
    st, win = sparse_store(name), SPARSE[name][1]
    eng.load(st.batch)
    for agg in GROUP_AGGS:
        for fn in DS_FUNS:
            check_paths(eng, st, query(win, agg, fn, INTERVAL), f"sparse {name} {agg}:{fn}", paths=SPARSE_PATHS)


def dev_figures(got, want):
    """(values that differ in bits, largest relative error) of two results of equal shape."""
    import numpy as np
    n = sum(int((np.asarray(b1) != np.asarray(b2)).sum()) for (_, _, b1, _), (_, _, b2, _) in zip(got, want))
    return n, V.max_rel_err(got, want)


@pytest.mark.parametrize("name", list(SPARSE))
def test_group_by_dev_over_missing_buckets(eng, sparse_store, name):
    """dev as the group-by aggregator, bit for bit like the other aggregators: the groups here hold
    two to five series, whose states reach the merge one value at a time in series order, and a
    merge of one value is the sequential recurrence's own step (ps_merge).  Groups whose tiles
    merge states of several values each keep the documented bound of 1e-9 and are not
    what this test is about.  The figure printed before the assertion is the number of values that
    differ in bits from the oracle and the largest relative error."""
    st, win = sparse_store(name), SPARSE[name][1]
    eng.load(st.batch)
    for fn in DS_FUNS:
        q = query(win, "dev", fn, INTERVAL)
        want, got = oracle_outcome(st.batch, q), engine_outcome(eng, q)
        if want[1] is None and got[1] is None:
            print(f"measured sparse {name} dev:{fn}: %d values differ in bits, max relative error %.3e" % dev_figures(got[0], want[0]))
        check_paths(eng, st, q, f"sparse {name} dev:{fn}", paths=SPARSE_PATHS)


@pytest.mark.parametrize("name", list(SPARSE))
def test_ordered_fold_over_missing_buckets(eng, sparse_store, name):
    """The ordered fold (query flag QF_ORDERED: the group's spans in SpanGroup order, one thread a
    slot) is the engine's bit-exact form of sum, avg and dev: over missing buckets too."""
    st, win = sparse_store(name), SPARSE[name][1]
    eng.load(st.batch)
    for agg in ("dev", "sum", "avg"):
        for fn in DS_FUNS:
            q = query(win, agg, fn, INTERVAL, flags=abi.QF_ORDERED)
            assert_same(engine_outcome(eng, q), oracle_outcome(st.batch, q), f"sparse {name} ordered {agg}:{fn}")


MULTI_AGGS = ["avg", "min", "max", "count", "dev"]


def multi_outcome(eng, qs, fuse):
    with options(MULTI_FUSE=fuse):
        try:
            return eng.run_multi(qs), None
        except EngineError as e:
            return None, e.java


def check_fused(eng, st, win, name, only):
    """run_multi of avg, min, max, count and dev (one shared pass, and query by query) against the
    oracle; asserts the results of the aggregators in `only`.  Where the oracle raises for one of
    the five the call raises the same exception, and the queries the oracle answers are then run
    by themselves.  The ZIM count of the fused pass equals the single-aggregator count query."""
    eng.load(st.batch)
    for fn in DS_FUNS:
        qs = [query(win, a, fn, INTERVAL) for a in MULTI_AGGS]
        want = [oracle_outcome(st.batch, q) for q in qs]
        errs = {w[1] for w in want} - {None}
        good = [i for i, w in enumerate(want) if w[1] is None]
        for fuse in (1, 0):
            ctx = f"sparse {name} run_multi {fn} MULTI_FUSE={fuse}"
            got, err = multi_outcome(eng, qs, fuse)
            if errs:
                assert err in errs, f"{ctx}: raised {err}, the oracle {errs}"
                got, err = multi_outcome(eng, [qs[i] for i in good], fuse) if good else ([], None)
            assert err is None, f"{ctx}: raised {err}"
            for i, g in zip(good, got):
                if MULTI_AGGS[i] not in only:
                    continue
                if MULTI_AGGS[i] == "dev":
                    print(f"measured {ctx} dev: %d values differ in bits, max relative error %.3e" % dev_figures(g, want[i][0]))
                V.assert_bits(g, want[i][0], f"{ctx} {MULTI_AGGS[i]}")
                if MULTI_AGGS[i] == "count":
                    single = engine_outcome(eng, qs[i])
                    assert single[1] is None
                    V.assert_bits(g, single[0], f"{ctx} count against the single query")


@pytest.mark.parametrize("name", list(SPARSE))
def test_fused_pass_over_missing_buckets(eng, sparse_store, name):
    check_fused(eng, sparse_store(name), SPARSE[name][1], name, ("avg", "min", "max", "count"))


@pytest.mark.parametrize("name", list(SPARSE))
def test_fused_pass_dev_over_missing_buckets(eng, sparse_store, name):
    """The dev output of the same run_multi calls, bit for bit."""
    check_fused(eng, sparse_store(name), SPARSE[name][1], name, ("dev",))


SEL_GROUP = [(f"SEL_WIN={w} SEL_COLS={c}", dict(SEL_WIN=w, SEL_COLS=c)) for w in (0, 2) for c in (0, 1)]


@pytest.mark.parametrize("name", list(SPARSE))
def test_percentile_group_by_over_missing_buckets(eng, sparse_store, name):
    st, win = sparse_store(name), SPARSE[name][1]
    eng.load(st.batch)
    for agg in ("p50", "p99", "median"):
        for fn in DS_FUNS:
            check_variants(eng, st, query(win, agg, fn, INTERVAL), f"sparse {name} {agg}:{fn}", [("default", {})] + SEL_GROUP)
