"""GPU parity at the value edges: the exactness certificate's threshold from both sides, sums
whose bits depend on the order, overflow at +-2^1023, signed zeros, NaN, +-Inf and a sweep of
scales -- through every downsample path (forced with the developer options, as test_gpu_fast.py
does), against the CPU oracle bit for bit, the sign of zero included (tests/value_edges.py:
assert_bits; no absolute floor anywhere).  tests/test_value_edges_cpu.py shows without a GPU
that the stores are as adversarial as they claim.

Which kernel a switch selects is shown where the data decides it: the certified stores stay in
the streaming kernels (fast_ms > 0, no tile handed back), the stores past the certificate do
not (redo_tiles > 0 or no streaming pass), k_hwin at 1m buckets over one-chunk rows and
k_seq_rows over six-point rows have tests of their own (selectors of tests/test_gpu_fast.py).

Tolerances of dev and squareSum (scale sweep): 4 x the largest relative error measured at scale
2^0 against the same statistic computed in exact rational arithmetic (fractions.Fraction, square
root in 60-digit decimal), by

    python -m pytest tests/test_gpu_value_edges.py -m gpu -k scale_sweep_dev -s

which prints "measured s=0 ..." before it asserts: 2.123e-16 for dev as a downsample function
(Welford in doubles against the exactly rounded value; under one ulp), 1.786e-16 for dev as the
group-by aggregator over three series, 0.0 for squareSum (40-bit squares of the dyadic base add
exactly); float32 and float64 cells alike.  A power-of-two scaling cannot change a relative
error, so the same bound holds at every scale whose squares neither underflow nor overflow.
"""
from __future__ import annotations

import decimal
import math
from fractions import Fraction

import numpy as np
import pytest

from opentsdb_amd import abi
from opentsdb_amd import engine as E
from opentsdb_amd.engine import EngineError, options
from oracle import oracle as O
from oracle import rollup as R
from tests import index_ref as IR
from tests import value_edges as V
from tests.test_gpu_parity import DEV_TOL, DS_FUNS

pytestmark = pytest.mark.gpu

T0, H = V.T0, V.H
DEV_EDGE_TOL = 4 * 2.123e-16
SQ_EDGE_TOL = 0.0
GROUP_DEV_EDGE_TOL = 4 * 1.786e-16

# every downsample path's switch (csrc/opts.h); a shape a path cannot take runs another one
PATHS = [("default", {}), ("SHORT=0", dict(SHORT=0)), ("ROWS=0", dict(ROWS=0)), ("HWIN=0", dict(HWIN=0)),
         ("HWIN=1", dict(HWIN=1)), ("SEQ=0", dict(SEQ=0)), ("SEQ_ROWS=0", dict(SEQ_ROWS=0)), ("SEQ_WAVE=0", dict(SEQ_WAVE=0)),
         ("SEQ_WAVE=1", dict(SEQ_WAVE=1)), ("SEQ_ROWS=1", dict(SEQ_ROWS=1)),
         # a scan with ROW_NOCERT rows goes to the sequential dense kernels first: without them the
         # streaming kernels (k_hwin at K > 64 over one-chunk rows, or the dense split) get it
         ("SEQ=0 HWIN=1", dict(SEQ=0, HWIN=1)), ("SEQ=0 HWIN=0", dict(SEQ=0, HWIN=0))]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def query(win, agg, fn, interval, **kw):
    return abi.new_query(win[0], win[1], agg, ds_function=abi.AGG[fn], ds_interval_ms=interval, **kw)


def oracle_outcome(batch, q):
    try:
        return O.run_query(batch, q), None
    except O.OracleError as e:
        return None, e.java


def engine_outcome(eng, q, **opts):
    """(result, java error name, timing) of the resident batch under the options."""
    with options(**opts):
        try:
            return eng.run(q), None, eng.timing()
        except EngineError as e:
            return None, e.java, None


def assert_same(got, want, ctx, cmp=V.assert_bits):
    (gr, ge), (wr, we) = got[:2], want[:2]
    assert ge == we, f"{ctx}: engine raised {ge}, oracle {we}"
    if we is None:
        cmp(gr, wr, ctx)


def check_paths(eng, store, q, ctx, paths=PATHS, cmp=V.assert_bits):
    """The resident store's query through k_grid (FAST = 0) and through every path of `paths`:
    each equals the oracle, and each equals k_grid bit for bit.  Returns the default path's timing."""
    want = oracle_outcome(store.batch, q)
    gen = engine_outcome(eng, q, FAST=0)
    assert_same(gen, want, f"{ctx} [FAST=0]", cmp)
    t_default = None
    for name, opts in paths:
        got = engine_outcome(eng, q, **opts)
        assert_same(got, want, f"{ctx} [{name}]", cmp)
        if want[1] is None:
            V.assert_bits(got[0], gen[0], f"{ctx} [{name}] against k_grid")
        if not opts:
            t_default = got[2]
    return t_default


def check_multi_and_ordered(eng, store, win, fn, interval, ctx):
    """The fused multi-aggregator pass (and the queries one by one), and the ordered fold."""
    aggs = ["min", "max", "count"]
    qs = [query(win, a, fn, interval) for a in aggs]
    want = [oracle_outcome(store.batch, q) for q in qs]
    if all(w[1] is None for w in want):
        for fuse in (1, 0):
            with options(MULTI_FUSE=fuse):
                got = eng.run_multi(qs)
            for a, g, w in zip(aggs, got, want):
                V.assert_bits(g, w[0], f"{ctx} run_multi {a} MULTI_FUSE={fuse}")
    q = query(win, "sum", fn, interval, flags=abi.QF_ORDERED)
    assert_same(engine_outcome(eng, q), oracle_outcome(store.batch, q), f"{ctx} ordered sum")


def not_order_free(t):
    return t.redo_tiles > 0 or t.fast_ms == 0


# ---- a. the certificate's threshold, both sides exact ---------------------------------------------
BOUNDARY = {**V.CERT_EXACT, **V.CERT_PAST}


@pytest.mark.parametrize("name", list(BOUNDARY))
def test_certificate_boundary(eng, name):
    make, interval, win = BOUNDARY[name]
    st = make()
    truth = V.series_truth(st, interval)
    eng.load(st.batch)
    for fn in ("sum", "avg"):
        for agg in ("none", "max"):
            t = check_paths(eng, st, query(win, agg, fn, interval), f"{name} {agg}:{fn}")
            if truth == "must_take_fast":
                assert t.fast_ms > 0 and t.redo_tiles == 0, f"{name} {agg}:{fn}: certified data left the order-free path"
            elif truth == "may_differ":
                assert not_order_free(t), f"{name} {agg}:{fn}: an order-free sum answered past the certificate"
    check_multi_and_ordered(eng, st, win, "sum", interval, name)


@pytest.mark.parametrize("shape,interval,win", [("one_row", 600000, (T0, T0 + H - 1)), ("walker", 60000, (T0, T0 + 2 * H - 1))])
@pytest.mark.parametrize("e", list(V.SQ_E))
def test_certificate_boundary_square_sum(eng, e, shape, interval, win):
    """squareSum doubles the exponent: odd integers under 2^e, squares under 2^(2e)."""
    st = V.odd_ints_store(e, shape)
    truth = V.series_truth(st, interval, square=True)
    assert truth == V.SQ_E[e]
    eng.load(st.batch)
    for agg in ("none", "max"):
        t = check_paths(eng, st, query(win, agg, "squareSum", interval), f"squareSum e{e} {shape} {agg}")
        if truth == "must_take_fast":
            assert t.fast_ms > 0 and t.redo_tiles == 0
        elif truth == "may_differ":
            assert not_order_free(t)


# ---- b. past the certificate: the order decides the bits ------------------------------------------
@pytest.mark.parametrize("name", list(V.CERT_MAY_DIFFER))
def test_order_dependent_sums_keep_javas_order(eng, name):
    make, interval, win = V.CERT_MAY_DIFFER[name]
    st = make()
    eng.load(st.batch)
    K = (win[1] - win[0]) * 1000 // interval + 1
    for fn in ("sum", "avg"):
        for agg in ("none", "max"):
            t = check_paths(eng, st, query(win, agg, fn, interval), f"{name} {agg}:{fn}")
            assert not_order_free(t), f"{name} {agg}:{fn}: an order-free sum answered"
    if K <= 64:
        check_multi_and_ordered(eng, st, win, "sum", interval, name)


# ---- which kernel answered: k_hwin and k_seq_rows (selectors and evidence of test_gpu_fast.py) -------
def test_hwin_takes_the_one_chunk_rows_at_1m(eng):
    """1m buckets over three one-chunk hour rows under a grouped aggregator (K = 180, 60 slots an
    hour) are k_hwin's: certified data stays in it (fast_ms > 0, no tile handed back); data whose
    rows certify but whose six-value buckets do not (7 * 2^48 + odd) is declined by k_hwin's own
    certificate at the series end (tiles handed back); ROW_NOCERT rows are handed back at once when
    the sequential dense kernels are off.  HWIN = 0 (the dense split) returns the same bits."""
    interval, win = V.HWIN_Q
    for name in ("odd_ints/e45/rows/1m", "f32_one_big/m15/rows/1m"):
        st = V.CERT_EXACT[name][0]()
        assert V.series_truth(st, interval) == "must_take_fast"
        eng.load(st.batch)
        for fn in ("sum", "avg"):
            q = query(win, "max", fn, interval)
            h = engine_outcome(eng, q, HWIN=1)
            d = engine_outcome(eng, q, HWIN=0)
            assert h[2].fast_ms > 0 and h[2].redo_tiles == 0, f"{name} {fn}: k_hwin handed {h[2].redo_tiles} tiles back"
            V.assert_bits(h[0], d[0], f"{name} {fn}: k_hwin against the dense split")
            V.assert_bits(h[0], O.run_query(st.batch, q), f"{name} {fn}: k_hwin against the oracle")
    st = V.CERT_MAY_DIFFER["band/rows/1m"][0]()
    eng.load(st.batch)
    _, flags, _, _ = eng.debug_rows()
    assert not (flags & IR.ROW_NOCERT).any()
    for fn in ("sum", "avg"):
        q = query(win, "max", fn, interval)
        h = engine_outcome(eng, q, HWIN=1)
        assert h[2].fast_ms > 0 and h[2].redo_tiles > 0, f"band {fn}: k_hwin's certificate did not decline"
        V.assert_bits(h[0], O.run_query(st.batch, q), f"band {fn}: k_hwin against the oracle")
    for name in ("big_odd52/rows/1m", "f32_mixed/rows/1m"):
        st = V.CERT_MAY_DIFFER[name][0]()
        eng.load(st.batch)
        _, flags, _, _ = eng.debug_rows()
        assert (flags & IR.ROW_NOCERT).all()
        q = query(win, "max", "sum", interval)
        assert engine_outcome(eng, q)[2].fast_ms == 0, f"{name}: the sequential dense kernels expected"
        h = engine_outcome(eng, q, SEQ=0, HWIN=1)
        assert h[2].fast_ms > 0 and h[2].redo_tiles == h[2].tiles, f"{name}: every tile handed back expected"
        V.assert_bits(h[0], O.run_query(st.batch, q), f"{name}: SEQ=0 HWIN=1 against the oracle")


@pytest.mark.parametrize("name", ["big_odd52/short/1h", "f32_mixed/short/1h", "overflow/short/1h"])
def test_seq_rows_takes_the_short_rows(eng, name):
    """Rows of six points with ROW_NOCERT values under buckets dividing the hour: k_seq_rows (one
    thread a row, Java's order), no streaming pass; SEQ_ROWS = 0 (k_seq_dense), SEQ_WAVE and SEQ = 0
    (k_grid) return the same bits, all the oracle's -- or its IllegalStateException."""
    st = V.overflow_store("short") if name.startswith("overflow") else V.CERT_MAY_DIFFER[name][0]()
    eng.load(st.batch)
    _, flags, _, _ = eng.debug_rows()
    assert (flags[:6] & IR.ROW_NOCERT).all()
    for interval in (3600000, 1800000, 1200000):
        for fn in ("sum", "avg"):
            for agg in ("max", "min", "none"):
                q = query(V.SHORT_WIN, agg, fn, interval)
                t = check_paths(eng, st, q, f"{name} {interval} {agg}:{fn}")
                if t is not None:
                    assert t.fast_ms == 0, f"{name} {interval} {agg}:{fn}: a streaming pass ran"


# ---- c. overflow ------------------------------------------------------------------------------------
OVERFLOW_SHAPES = [("one_row", 600000), ("rows", 600000), ("walker", 60000), ("rows", 60000), ("short", 3600000)]


@pytest.mark.parametrize("shape,interval", OVERFLOW_SHAPES)
def test_overflow_bucket(eng, shape, interval):
    """[M, M, -M, -M] x 15, M = 2^1023: Java's order gives +Inf.  52 + lsb = 1075 is past the
    exponent range: a certificate written as n * A <= ldexp(1, 52 + lsb) compares inf <= inf."""
    win = (T0, T0 + V.SHAPES[shape][0] * H - 1)
    st = V.overflow_store(shape)
    eng.load(st.batch)
    ndp, flags, lsb, amax = eng.debug_rows()
    rn, rf, rl, ra, _ = IR.index_ref(st.batch)
    np.testing.assert_array_equal(ndp, rn)
    np.testing.assert_array_equal(lsb, rl)
    np.testing.assert_array_equal(amax, ra)
    np.testing.assert_array_equal(flags & np.uint32(0xFFFFFFFF ^ IR.ROW_SFIRST), rf)
    assert flags[0] & IR.ROW_NOCERT and lsb[0] == 1023 and amax[0] == V.HUGE
    if V.per_bucket(shape, interval) % 4 == 0:   # every bucket starts M, M: +Inf beside the partner's count
        want = oracle_outcome(st.batch, query(win, "min", "sum", interval))
        assert want[1] is None and set(np.asarray(want[0][0][2]).view(np.float64)) == {float(V.per_bucket(shape, interval))}
    for agg in ("min", "max", "count"):
        for fn in ("sum", "avg"):
            check_paths(eng, st, query(win, agg, fn, interval), f"overflow {shape} {agg}:{fn}")
    check_multi_and_ordered(eng, st, win, "sum", interval, f"overflow {shape}")
    alone = V.overflow_store(shape, partner=False)
    eng.load(alone.batch)
    for agg in ("sum", "avg", "none"):
        for fn in ("sum", "avg"):
            q = query(win, agg, fn, interval)
            assert oracle_outcome(alone.batch, q)[1] == "IllegalStateException"   # (some bucket overflows in every shape)
            check_paths(eng, alone, q, f"overflow alone {shape} {agg}:{fn}")


@pytest.mark.parametrize("shape,interval", OVERFLOW_SHAPES)
@pytest.mark.parametrize("stride", V.OVERFLOW_STRIDES)
def test_overflow_arrangements(eng, stride, shape, interval):
    """+-2^1023 in arrangements where Java's order overflows and a sum by lanes or pairs cancels,
    and the other way round: the oracle's bits, or its IllegalStateException, on every path."""
    win = (T0, T0 + V.SHAPES[shape][0] * H - 1)
    outcomes = set()
    for pattern in V.OVERFLOW_PATTERNS:
        st = V.overflow_pattern_store(pattern, stride, shape)
        eng.load(st.batch)
        for agg, fn in (("min", "sum"), ("none", "sum"), ("min", "avg")):
            q = query(win, agg, fn, interval)
            outcomes.add(oracle_outcome(st.batch, q)[1])
            check_paths(eng, st, q, f"overflow {pattern} stride {stride} {shape} {agg}:{fn}")
    if V.per_bucket(shape, interval) >= 60:   # (six-cell buckets at a stride of 8 or 15 hold one +-M at most)
        assert outcomes == {None, "IllegalStateException"}


# ---- d. signed zero -----------------------------------------------------------------------------------
ZERO_FUNS = ["min", "max", "first", "last", "sum", "avg"]


@pytest.mark.parametrize("first_sign", [1.0, -1.0])
@pytest.mark.parametrize("kind", [V.F32, V.F64])
@pytest.mark.parametrize("shape", ["one_row", "rows", "walker"])
def test_signed_zero_inside_a_bucket(eng, shape, kind, first_sign):
    """Java folds min / max with x < m: of +0.0 and -0.0 the one met first stays."""
    st = V.zeros_store(kind, first_sign, shape)
    eng.load(st.batch)
    win = (T0, T0 + V.SHAPES[shape][0] * H - 1)
    for fn in ZERO_FUNS:
        check_paths(eng, st, query(win, "none", fn, 60000), f"zeros {shape} kind {kind} {first_sign:+} none:{fn}")
    check_paths(eng, st, query(win, "none", "min", 1000), f"zeros {shape} K > 64")
    for agg in ("min", "max"):   # one series a group: grouped queries (rows at 1m over 3 h: k_hwin's shape)
        for fn in ZERO_FUNS:
            check_paths(eng, st, query(win, agg, fn, 60000), f"zeros {shape} kind {kind} {first_sign:+} {agg}:{fn}")


ZERO_GROUPS = {
    "+-": [1, -1], "-+": [-1, 1], "+--+-": [1, -1, -1, 1, -1], "-++-+": [-1, 1, 1, -1, 1],
    "129+ then -": [1] * 129 + [-1], "- then 129+": [-1] + [1] * 129, "70- then 70+": [-1] * 70 + [1] * 70,
    "70+ then 70-": [1] * 70 + [-1] * 70,
}


@pytest.mark.parametrize("name", list(ZERO_GROUPS))
def test_signed_zero_across_series(eng, name):
    """Group-by over series whose buckets are +0.0 / -0.0: the first series met decides min / max;
    130 and 140 series span tiles, so k_reduce resolves the tie."""
    st = V.zero_groups_store(ZERO_GROUPS[name])
    eng.load(st.batch)
    win = (T0, T0 + H - 1)
    for agg in ("min", "max", "sum", "avg", "first", "last", "mimmin", "mimmax"):
        for fn in ("min", "first"):
            check_paths(eng, st, query(win, agg, fn, 600000), f"zero groups {name} {agg}:{fn}", paths=PATHS[:2])
    check_multi_and_ordered(eng, st, win, "min", 600000, f"zero groups {name}")


@pytest.mark.parametrize("name", ["-+", "70- then 70+", "70+ then 70-"])
def test_signed_zero_across_devices(name):
    """Series-shard mode on two contexts of one device: the merge across devices sees the tie."""
    st = V.zero_groups_store(ZERO_GROUPS[name])
    e = E.Engine(devices=[0, 0])
    try:
        e.shard_mode(E.SHARD_SERIES)
        e.load(st.batch)
        for agg in ("min", "max", "sum"):
            q = query((T0, T0 + H - 1), agg, "min", 600000)
            V.assert_bits(e.run(q), O.run_query(st.batch, q), f"two devices {name} {agg}")
    finally:
        e.close()


# ---- e. NaN -----------------------------------------------------------------------------------------------
NAN_CASES = ["bucket", "series", "bucket_first", "series_first", "row"]
NAN_AGGS = ["sum", "min", "max", "count", "dev", "none"]


@pytest.fixture(scope="module")
def nan_stores():
    return {(c, k): V.nan_store(c, k) for c in NAN_CASES for k in (V.F32, V.F64)}


@pytest.mark.parametrize("fn", DS_FUNS)
@pytest.mark.parametrize("case", NAN_CASES)
def test_nan_cells(eng, nan_stores, case, fn):
    win = (T0, T0 + 3 * H - 1)
    for kind in (V.F32, V.F64):
        st = nan_stores[(case, kind)]
        eng.load(st.batch)
        for agg in NAN_AGGS:
            cmp = (lambda g, w, c: V.assert_rel(g, w, DEV_TOL, c)) if "dev" in (agg, fn) else V.assert_bits
            for kw in (dict(), dict(ds_fill=abi.FILL_NAN), dict(ds_fill=abi.FILL_ZERO), dict(rate=True)):
                q = query(win, agg, fn, 60000, **kw)
                ctx = f"nan {case} kind {kind} {agg}:{fn} {kw}"
                want = oracle_outcome(st.batch, q)
                for name, opts in (("FAST=0", dict(FAST=0)), ("default", {}), ("ROWS=0", dict(ROWS=0))):
                    assert_same(engine_outcome(eng, q, **opts), want, f"{ctx} [{name}]", cmp)


# ---- f. infinity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signs", [(1,), (-1,), (1, -1), (-1, 1)], ids=["+inf", "-inf", "+inf,-inf", "-inf,+inf"])
@pytest.mark.parametrize("kind", [V.F32, V.F64])
@pytest.mark.parametrize("shape", ["one_row", "rows", "walker"])
def test_infinite_cells(eng, shape, kind, signs):
    """An infinity a group-by absorbs (count; min / max beside a finite partner) gives the oracle's
    bits; one that reaches an output raises IllegalStateException on both sides; +Inf and -Inf in
    one bucket sum to NaN."""
    win = (T0, T0 + V.SHAPES[shape][0] * H - 1)
    raised = absorbed = 0
    for partner in (True, False):
        st = V.inf_store(signs, kind, shape, partner)
        eng.load(st.batch)
        for agg in ("count", "min", "max", "sum", "none"):
            for fn in ("sum", "avg", "min", "max", "first", "count"):
                q = query(win, agg, fn, 60000)
                check_paths(eng, st, q, f"inf {signs} {shape} kind {kind} partner {partner} {agg}:{fn}")
                err = oracle_outcome(st.batch, q)[1]
                assert err in (None, "IllegalStateException")
                raised += err is not None
                absorbed += err is None
        for fn in ("sum", "min"):
            check_multi_and_ordered(eng, st, win, fn, 60000, f"inf {signs} {shape} kind {kind} partner {partner} {fn}")
    assert raised and absorbed
    if len(signs) == 2:
        st = V.inf_store(signs, kind, shape, partner=False)
        (_, ts, bits, _), = O.run_query(st.batch, query(win, "none", "sum", 60000))
        assert np.isnan(np.asarray(bits).view(np.float64)[3])


# ---- g. the scale sweep -----------------------------------------------------------------------------------
SWEEP_FUNS = ["sum", "avg", "min", "max", "count", "first", "last", "diff"]
WIN1 = (T0, T0 + H - 1)
SWEEP_SHAPES = {"one_row": 600000, "rows": 600000, "walker": 60000}   # 60 points a bucket


def sweep_win(shape):
    return (T0, T0 + V.SHAPES[shape][0] * H - 1)


def sweep_queries(shape="one_row"):
    """(name, query): each function as the downsample function under group-by none, and as the
    group-by aggregator over sum-downsampled buckets."""
    win, iv = sweep_win(shape), SWEEP_SHAPES[shape]
    qs = [(f"none:{f}", query(win, "none", f, iv)) for f in SWEEP_FUNS]
    return qs + [(f"{a}:sum", query(win, a, "sum", iv)) for a in SWEEP_FUNS]


@pytest.fixture(scope="module")
def sweep_base(eng):
    """The s = 0 results of the engine and of the oracle, by kind and shape."""
    out = {}
    for kind in (V.F64, V.F32):
        for shape in SWEEP_SHAPES:
            st = V.scaled_store(0, kind, shape=shape)
            eng.load(st.batch)
            out[kind, shape] = {n: (eng.run(q), O.run_query(st.batch, q)) for n, q in sweep_queries(shape)}
    return out


@pytest.mark.parametrize("shape", list(SWEEP_SHAPES))
@pytest.mark.parametrize("kind,s", [(V.F64, s) for s in V.SCALES_F64] + [(V.F32, s) for s in V.SCALES_F32])
def test_scale_sweep(eng, sweep_base, kind, s, shape):
    st = V.scaled_store(s, kind, shape=shape)
    eng.load(st.batch)
    pure = 0
    for name, q in sweep_queries(shape):
        ctx = f"scale 2^{s} kind {kind} {shape} {name}"
        check_paths(eng, st, q, ctx)
        want = oracle_outcome(st.batch, q)
        got = engine_outcome(eng, q)
        g0, w0 = sweep_base[kind, shape][name]
        if want[1] is None and V.is_pure_scaling(w0, want[0], s):   # decided from the oracle alone
            assert V.is_pure_scaling(g0, got[0], s), f"{ctx}: not 2^s x the s = 0 result"
            pure += 1
    for fn in ("sum", "min"):
        check_multi_and_ordered(eng, st, sweep_win(shape), fn, SWEEP_SHAPES[shape], f"scale 2^{s} kind {kind} {shape} {fn}")
    if s > -1000 and not (kind == V.F32 and s < -126):   # (below: subnormal cells round anew)
        assert pure >= 10, f"scale 2^{s} kind {kind} {shape}: only {pure} queries scale purely in the oracle"


@pytest.mark.parametrize("shape", list(SWEEP_SHAPES))
def test_long_cells_near_2_63(eng, shape):
    """8-byte integer cells +-(2^62 + odd): integer arithmetic, bit for bit (sums wrap as Java's)."""
    st = V.long_store(shape=shape)
    eng.load(st.batch)
    for name, q in sweep_queries(shape):
        check_paths(eng, st, q, f"longs {shape} {name}")
    check_multi_and_ordered(eng, st, sweep_win(shape), "sum", SWEEP_SHAPES[shape], f"longs {shape}")


def _sqrt_fraction(x: Fraction) -> float:
    if x == 0:
        return 0.0
    with decimal.localcontext() as c:
        c.prec = 60
        c.Emax, c.Emin = 999999, -999999
        return float((decimal.Decimal(x.numerator) / decimal.Decimal(x.denominator)).sqrt())


def exact_buckets(store, fn, like, group=False):
    """dev / squareSum of every series' 600 s buckets in exact rational arithmetic, rounded once, in
    the shape of the result `like` (group-by none); group: the population deviation, per group and
    bucket, of the member series' exact bucket sums (dev as the group-by aggregator over sum)."""
    per = []
    for ts, v, _ in store.series:
        vals = []
        for b in V.buckets_of(ts, v, 600000).values():
            fr = [Fraction(x) for x in b]
            if group:
                vals.append(sum(fr))
            elif fn == "squareSum":
                x = sum(f * f for f in fr)
                vals.append(x.numerator / x.denominator)   # (int / int rounds correctly)
            else:
                mean = sum(fr) / len(fr)
                vals.append(_sqrt_fraction(sum((f - mean) ** 2 for f in fr) / len(fr)))
        per.append(vals)
    out = []
    if not group:
        for vals, (g, t, bits, isint) in zip(per, like):
            assert len(vals) == len(t)
            out.append((g, t, np.array(vals, np.float64).view(np.uint64), isint))
        return out
    for g, t, bits, isint in like:
        members = [per[i] for i, gid in enumerate(store.gids) if gid == g]
        vals = []
        for k in range(len(t)):
            xs = [m[k] for m in members]
            mean = sum(xs) / len(xs)
            vals.append(_sqrt_fraction(sum((x - mean) ** 2 for x in xs) / len(xs)))
        out.append((g, t, np.array(vals, np.float64).view(np.uint64), isint))
    return out


# squares of the scaled base span 2^(2s - 20) .. 2^(2s + 20): neither under- nor overflow here
REL_SCALES = {V.F64: [s for s in V.SCALES_F64 if abs(2 * s) + 20 < 1000],
              V.F32: [s for s in V.SCALES_F32 if s > -126 + 10]}   # (float32 cells: normal numbers only)
EDGE_TOL = {"none:dev": DEV_EDGE_TOL, "none:squareSum": SQ_EDGE_TOL, "dev:sum": GROUP_DEV_EDGE_TOL}


@pytest.mark.parametrize("kind", [V.F64, V.F32])
@pytest.mark.parametrize("level", list(EDGE_TOL))
def test_scale_sweep_dev_and_square_sum(eng, level, kind):
    """True relative error against exact arithmetic, the same bound at every scale: dev and
    squareSum as downsample functions, dev as the group-by aggregator (three series a group)."""
    agg, fn = level.split(":")
    tol = EDGE_TOL[level]
    assert REL_SCALES[V.F64] == [-140, -100, -40, 0, 40, 100] and REL_SCALES[V.F32] == [-100, -40, 0, 40, 100]
    for s in [0] + [x for x in REL_SCALES[kind] if x]:
        st = V.scaled_store(s, kind)
        eng.load(st.batch)
        q = query(WIN1, agg, fn, 600000)
        got = eng.run(q)
        ref = exact_buckets(st, fn, got, group=agg == "dev")
        err = V.max_rel_err(got, ref)
        print(f"measured s={s} {level} kind {kind}: max relative error {err:.3e} against exact arithmetic (bound {tol:.3e})")
        V.assert_rel(got, ref, tol, f"{level} at 2^{s} against exact arithmetic")
        V.assert_rel(O.run_query(st.batch, q), ref, tol, f"oracle {level} at 2^{s} against exact arithmetic")
        V.assert_rel(engine_outcome(eng, q, FAST=0)[0], ref, tol, f"{level} at 2^{s} [FAST=0]")


@pytest.mark.parametrize("s", [-600, 600, -1060, 960])
def test_square_sum_under_and_overflow(eng, s):
    """Squares that underflow to zero or overflow to +Inf: the oracle's bits or its exception
    (the certificate's low exponent guard and its overflow case are the code under test)."""
    st = V.scaled_store(s)
    eng.load(st.batch)
    for agg in ("none", "max", "count"):
        check_paths(eng, st, query(WIN1, agg, "squareSum", 600000), f"squareSum at 2^{s} {agg}")


# ---- rollup generation ------------------------------------------------------------------------------------
ROLLUP_FUNCS = (("sum", 0), ("count", 1), ("max", 2), ("min", 3))


def rollup_outcome_oracle(batch, interval, span, start, end):
    try:
        return R.generate(batch, R.Interval(interval, span), start, end, ROLLUP_FUNCS), None
    except R.RollupError:
        return None, "IllegalArgumentException"


def check_rollup(eng, store, rows, ctx):
    eng.load(store.batch)
    for interval, span in (("1h", "1d"), ("10m", "1d")):
        want, werr = rollup_outcome_oracle(store.batch, interval, span, T0, T0 + rows * H)
        try:
            cells = eng.rollup(E.rollup_interval(interval, span), T0, T0 + rows * H, ROLLUP_FUNCS)
            got, gerr = [cells.cell(i) for i in range(len(cells))], None
        except EngineError as e:
            got, gerr = None, e.java
        assert gerr == werr, f"{ctx} {interval}: engine raised {gerr}, oracle {werr}"
        if werr is None:
            assert len(got) == len(want), f"{ctx} {interval}"
            for i, (g, w) in enumerate(zip(got, want)):
                assert g == w, (ctx, interval, i, g, w)


ROLLUP_STORES = {
    "odd_ints e45": (lambda: V.odd_ints_store(45, "walker"), 2),
    "odd_ints e47": (lambda: V.odd_ints_store(47, "walker"), 2),
    "odd_ints e48": (lambda: V.odd_ints_store(48, "walker"), 2),
    "big_odd one_row": (lambda: V.big_odd_store("one_row"), 1),
    "big_odd walker": (lambda: V.big_odd_store("walker"), 2),
    "f32_mixed walker": (lambda: V.f32_mixed_store("walker"), 2),
    "cross_row": (lambda: V.cross_row_store(), 2),          # (1h cells stay inside a row; the 1d cells are below)
    "zeros f32 +": (lambda: V.zeros_store(V.F32, 1.0), 1),
    "zeros f64 -": (lambda: V.zeros_store(V.F64, -1.0), 1),
    "dyadic walker f64": (lambda: V.scaled_store(0, V.F64, shape="walker"), 2),   # certified rows of 3600 points
    "dyadic walker f32": (lambda: V.scaled_store(0, V.F32, shape="walker"), 2),
    "overflow with partner": (lambda: V.overflow_store("one_row"), 1),
    "overflow walker": (lambda: V.overflow_store("walker", partner=False), 2),
    "overflow M-M-MM stride 15": (lambda: V.overflow_pattern_store("M-M-MM", 15, "rows"), 3),
    "overflow -MMM-M stride 8": (lambda: V.overflow_pattern_store("-MMM-M", 8, "walker"), 2),
    "overflow MM-M-M-M-MMM stride 2": (lambda: V.overflow_pattern_store("MM-M-M-M-MMM", 2, "one_row"), 1),
}


@pytest.mark.parametrize("name", list(ROLLUP_STORES))
def test_rollup_cells_at_the_value_edges(eng, name):
    """Rollup generation (1h and 10m cells) byte for byte against oracle.rollup.generate; an
    infinite sum is rejected on both sides.

    "overflow -MMM-M stride 8" and the dyadic walker stores pin k_rollup_fast's count of a row
    longer than one chunk inside one bucket: a series of the launch that passes the certificate
    beside one that is handed back (or simply 1 s rows of small dyadic values under 1h cells)."""
    make, rows = ROLLUP_STORES[name]
    check_rollup(eng, make(), rows, f"rollup {name}")


def test_rollup_cross_row_day_cells(eng):
    """Cells of one day: both hour rows of the cross-row store fall into one bucket."""
    st = V.cross_row_store()
    eng.load(st.batch)
    want = R.generate(st.batch, R.Interval("1d", "1n"), T0, T0 + 2 * H, ROLLUP_FUNCS)
    cells = eng.rollup(E.rollup_interval("1d", "1n"), T0, T0 + 2 * H, ROLLUP_FUNCS)
    got = [cells.cell(i) for i in range(len(cells))]
    assert got == want
