"""GPU parity of percentile / median downsampling at the size and rank edges of every route of
csrc/k_pct.hip: the stores of tests/pct_edges.py (proved on the host by
tests/test_pct_edges_cpu.py) against the oracle under the group-by aggregator `none` at tol 0 --
every series' bucket values bit for bit --, for p999, p99, p95, p90, p75, p50, median and ep99r7,
with the route asserted from Engine.debug_pct() against pct_edges.predict: (k_pct_rows launched,
its KEYS variant, series it handed back, series sent to the large-bucket pass, that pass's waves),
and big_cap at least the largest series' in-range datapoints.

Families B (one row class a store, rows on the rank and extraction edges) and E (signed zeros and
infinities on the ranks) run under the default options and with PCT_V6, PCT_VONLY, PCT_KEYS and
PCT_ROWS off in turn: five routes, all bit-identical to the oracle and so to each other.  A
function whose rank lands on an infinity raises IllegalStateException on both sides (family E's
inf stores); there the outcome is what is compared."""
from __future__ import annotations

import pytest

from opentsdb_amd.engine import EngineError, options
from oracle import oracle as O
from tests import pct_edges as P
from tests.test_gpu_parity import assert_groups_match

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from opentsdb_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def prepared():
    cache = {}

    def get(name):
        if name not in cache:
            case = P.CASES[name]()
            cache[name] = (case, P.prepare(case.store), {})
        return cache[name]
    return get


def oracle_outcome(case, fn, agg, memo):
    if (fn, agg) not in memo:
        try:
            memo[(fn, agg)] = (O.run_query(case.store, P.query(case, fn, agg)), None)
        except O.OracleError as e:
            memo[(fn, agg)] = (None, e.java)
    return memo[(fn, agg)]


def engine_outcome(eng, q, load=None):
    try:
        return (eng.run_batch(load, q) if load is not None else eng.run(q)), None
    except EngineError as e:
        return None, e.java


def check(eng, prepared, name, option_sets=({},), fns=P.FUNCS, errors=False):
    """Every function of `fns` over the case under every option set: the oracle's bits (or its
    exception, where `errors` allows one) and the predicted route; then max and count once."""
    case, prep, memo = prepared(name)
    raised = 0
    for fn in fns:
        want, want_err = oracle_outcome(case, fn, "none", memo)
        assert errors or want_err is None, (fn, want_err)
        raised += want_err is not None
        for i, opts in enumerate(option_sets):
            with options(**opts):
                got, got_err = engine_outcome(eng, P.query(case, fn), case.store if i == 0 else None)
                route = eng.debug_pct()
            pred = P.predict(case.store, case.win, case.I, fn, opts, prep)
            ctx = f"{name} {fn} {opts or 'default'}"
            print(f"{ctx}: route {route}, predicted {pred.readout()} cap >= {pred.cap_min}, "
                  f"back {sorted(set(pred.back.values()))}, oracle {want_err}, engine {got_err}")
            assert got_err == want_err, ctx
            if want is not None:
                assert_groups_match(got, want, "none", tol=0.0, ctx=ctx)
            assert route[:5] == pred.readout(), ctx
            assert route[5] >= pred.cap_min if pred.big else route[5] == 0, ctx
    for fn in fns:
        for agg in ("max", "count"):
            want, want_err = oracle_outcome(case, fn, agg, memo)
            got, got_err = engine_outcome(eng, P.query(case, fn, agg))
            assert got_err == want_err, (name, fn, agg)
            if want is not None:
                assert_groups_match(got, want, agg, tol=0.0, ctx=f"{name} {fn} {agg}")
    return raised


# ---- A: size classes (k_pct over every series) ------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.A_CASES))
def test_a_size_classes(eng, prepared, name):
    """3 h buckets of 1 .. 8193 kept values: both bitonic sorts at 511 .. 513, 1023 .. 1025,
    2047 .. 2049, 4095 / 4096, the spill and the radix select from 4097, a small bucket after a large
    one in the same LDS buffer and spill region; with NaNs, raw counts that cross a threshold the
    kept count does not."""
    check(eng, prepared, name)
    case, prep, _ = prepared(name)
    pred = P.predict(case.store, case.win, case.I, "p99", prep=prep)
    assert pred.launched == 0 and len(pred.big) == len(case.classes)


# ---- B: rank edges inside k_pct_rows -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.B_CASES))
def test_b_rank_edges_every_route(eng, prepared, name):
    check(eng, prepared, name, P.OPTION_SETS)
    case, prep, _ = prepared(name)
    variants = {P.predict(case.store, case.win, case.I, fn, o, prep).variant for fn in ("p99", "median") for o in P.OPTION_SETS}
    four = case.classes[0][1] == 4
    if name in ("q2f4_384", "q4f4_384"):
        assert variants == {13, 14, 5, 6, 1, 2, 0, -1}
    elif name == "mixed4":
        assert variants == {1, 2, 0, -1}
    elif four:
        assert variants == {5, 6, 1, 2, 0, -1}
    else:
        assert variants == {0, -1}


# ---- C: sub-hour slots ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.C_CASES))
def test_c_sub_hour_slots(eng, prepared, name):
    """Millisecond offsets one either side of, and on, every bucket boundary of an hour row, under
    intervals whose float reciprocal is exact (1000, 45 000, 60 000, 1 800 000 ms) and inexact
    (1125, 9375): decode_row's quotient and its corrections; with PCT_ROWS off, k_pct's own slots."""
    check(eng, prepared, name, ({}, {"PCT_ROWS": 0}))
    case, prep, _ = prepared(name)
    assert P.predict(case.store, case.win, case.I, "p90", prep=prep).readout() == (1, 0, 0, 0, 0)


# ---- D: the chain -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.D_CASES))
def test_d_chain(eng, prepared, name):
    """k_pct_rows -> k_pct over its hand-backs -> the large-bucket pass (LDS sort at 3600, radix
    select at 4097) in one query, with 1 .. 4 series in that pass (2, 2, 4, 4 waves)."""
    check(eng, prepared, name)
    case, prep, _ = prepared(name)
    pred = P.predict(case.store, case.win, case.I, "p99", prep=prep)
    n1s = int(name[-1])
    assert (pred.launched, pred.variant, len(pred.back), len(pred.big)) == (1, 13, n1s + 2, n1s + 1)


# ---- E: signed zeros and infinities ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.E_CASES))
def test_e_signed_zeros_every_route(eng, prepared, name):
    """The requested rank on a zero next to a zero of the other sign, in buckets of 9 .. 4097
    values: the key kernel, the extraction, both bitonic sorts and the radix select must all order
    -0.0 before 0.0, as Double.compareTo does."""
    assert check(eng, prepared, name, P.OPTION_SETS) == 0


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("n", P.E_INF_SIZES)
def test_e_infinities_every_route(eng, prepared, f64, n):
    """Buckets that hold the extraction's own "removed" markers, +-Inf, on and next to the ranks:
    the values, or IllegalStateException where an infinity reaches an output, as the oracle has it."""
    raised = 0
    for kind in P.E_INF_KINDS:
        for fn in P.E_INF_FUNCS:
            raised += check(eng, prepared, f"inf_{'f64' if f64 else 'f32'}_{n}_{kind}_{fn}", P.OPTION_SETS, errors=True)
    assert raised > 0


# ---- the read-out ------------------------------------------------------------------------------------------------------
def test_debug_pct_before_any_run_and_on_two_devices():
    from opentsdb_amd import engine
    e = engine.Engine(0)
    try:
        assert e.debug_pct() == (0, -1, 0, 0, 0, 0)
    finally:
        e.close()
    md = engine.Engine(devices=[0, 0])
    try:
        with pytest.raises(EngineError) as ei:
            md.debug_pct()
        assert ei.value.java == "NotImplemented"
    finally:
        md.close()
