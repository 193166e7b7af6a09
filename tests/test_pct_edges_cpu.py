"""The stores of tests/pct_edges.py are what they claim (no GPU): the non-NaN count of every
(series, bucket) and every row's class, counted from the bytes; the plain restatement of a
bucket's value against the oracle bit for bit, for p999 .. p50, median and ep99r7; the rank and
extraction edges the sizes are named for; and the route predictor on hand-worked cases."""
from __future__ import annotations

import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import index_ref as IR
from tests import pct_edges as P


@pytest.fixture(scope="module")
def prepared():
    cache = {}

    def get(name):
        if name not in cache:
            case = P.CASES[name]()
            cache[name] = (case, P.prepare(case.store))
        return cache[name]
    return get


# ---- the restatement itself -------------------------------------------------------------------------
def test_bucket_value_hand_worked():
    assert math.isnan(P.bucket_value([], "p99")) and math.isnan(P.bucket_value([math.nan], "median"))
    assert P.bucket_value([7.0], "p50") == 7.0
    assert P.bucket_value([4, 1, 3, 2], "median") == 3.0                 # sorted[4 // 2]
    assert P.bucket_value([4, 1, 3, 2], "p50") == 2.5                    # pos = 2.5
    assert P.bucket_value([4, 1, math.nan, 3, 2], "p75") == 3.75         # pos = 3.75: 3 + 0.75 (4 - 3)
    assert P.bucket_value(range(1, 10), "p90") == 9.0                    # pos = 9 >= n: the maximum
    assert P.bucket_value(range(1, 11), "p90") == 9.9                    # pos = 9.9: 9 + 0.9 (10 - 9)
    v = list(range(1000))
    pos = (99.9 / 100.0) * 1001                                          # not exact in binary (and not 0.999 * 1001)
    assert 999 < pos < 1000 and P.bucket_value(v, "p999") == 998 + (pos - 999) * (999 - 998)
    assert P.bucket_value(v[:999], "p999") == 998.0
    # the total order: -0.0 before 0.0
    z = P.bucket_value([0.0, -0.0, 0.0, -0.0], "median")                 # sorted: -0 -0 +0 +0, index 2
    assert z == 0 and math.copysign(1, z) == 1
    z = P.bucket_value([0.0, -0.0, -0.0], "median")                      # sorted: -0 -0 +0, index 1
    assert z == 0 and math.copysign(1, z) == -1
    z = P.bucket_value([0.0, -0.0, 5.0], "p50")                          # pos = 2: -0.0 + 0 * (0.0 - -0.0) = -0.0 + 0.0 = +0.0
    assert z == 0 and math.copysign(1, z) == 1
    assert math.isnan(P.bucket_value([1.0, math.inf, math.inf], "p50"))  # Inf + 0 * (Inf - Inf)


CLAMP_UNTIL = {"p999": 999, "p99": 99, "p95": 19, "p90": 9, "p75": 3, "p50": 1, "ep99r7": 99}
EXTRACT_UNTIL = {"p999": 512, "p99": 512, "p95": 479, "p90": 239, "p75": 95, "p50": 47, "median": 48, "ep99r7": 512}


@pytest.mark.parametrize("fn", P.FUNCS)
def test_rank_and_extraction_edges(fn):
    """The sizes the stores are named for: pos >= n up to CLAMP_UNTIL, one size later two ranks; a
    statistic within 24 of an end up to EXTRACT_UNTIL (of the sizes up to 512), beyond it one size later."""
    if fn != "median":
        n = CLAMP_UNTIL[fn]
        assert P.ranks(fn, n)[:2] == (n - 1, n - 1)
        lo, hi, pos = P.ranks(fn, n + 1)
        assert (lo, hi) == (n - 1, n) and n <= pos < n + 1
        assert n in P.SIZES and n + 1 in P.SIZES
    n = EXTRACT_UNTIL[fn]
    assert all(not P._far(fn, m) for m in range(1, n + 1))
    assert n == 512 or P._far(fn, n + 1)
    assert n in P.SIZES and (n == 512 or n + 1 in P.SIZES)
    assert {511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097} <= set(P.SIZES)
    assert {383, 384, 385} <= set(P.ROW_SIZES) and max(P.ROW_SIZES) == 512


# ---- the stores ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.CASES))
def test_store_counts_and_classes(prepared, name):
    case, _prep = prepared(name)
    dec = P.decode(case.store)
    assert P.non_nan_counts(case.store, case.win, case.I, dec) == case.counts
    _ndp, flags, _lsb, _amax, facts = IR.index_ref(case.store)
    r = 0
    for s, rows in enumerate(dec):
        for _base, _ts, _xs, qws, vls, _isf in rows:
            f = facts[r]
            assert not f.err and not int(flags[r]) & IR.ROW_UNSORTED, (s, r)
            if case.classes[s] is not None:
                assert set(qws) == {case.classes[s][0]} and set(vls) == {case.classes[s][1]}, (s, r, set(qws), set(vls))
                assert (f.qw, f.vl) == case.classes[s]
            r += 1


def test_size_stores_hold_every_size():
    for nans in (False, True):
        case = P.sizes_case(nans)
        ns = len(case.classes)
        for s in range(ns):
            got = sorted(n for (ss, _b), n in case.counts.items() if ss == s and n)
            assert got == sorted(P.SIZES)
        # a small bucket after a large one, an empty bucket between two full ones, two hour rows above 3600
        order = P.size_order()
        assert any(a is not None and b is not None and a > 4096 and b <= 4 for a, b in zip(order, order[1:]))
        i = order.index(None)
        assert order[i - 1] and order[i + 1]
    dec = P.decode(P.sizes_case(True).store)
    raw = {}
    for rows in dec[:1]:
        for _base, ts, xs, *_ in rows:
            for t, x in zip(ts.tolist(), xs.tolist()):
                k = t - t % P.A_I
                a, b = raw.get(k, (0, 0))
                raw[k] = (a + 1, b + (x == x))
    assert {(520, 512), (4100, 4096), (4200, 4097), (5, 0)} <= set(raw.values())


def test_rank_stores_hold_the_edge_values():
    for qw in (2, 4):
        case = P.rank_case(qw, "i4")
        dec = P.decode(case.store)
        per_series = [np.concatenate([xs for _b, _t, xs, *_ in rows]) for rows in dec]
        assert P.INT32_MAX in per_series[3] and P.INT32_MIN + 1 in per_series[3] and P.INT32_MIN not in per_series[3]
        assert P.INT32_MIN in per_series[4]
        assert all(P.INT32_MIN not in x for x in per_series[:3])
    longest = lambda c: max(len(r[1]) for rows in P.decode(c.store) for r in rows)      # noqa: E731
    assert longest(P.B_CASES["q2f4_384"]()) == 384 and longest(P.B_CASES["q2f4_385"]()) == 385
    assert longest(P.B_CASES["q2f4"]()) == 512


@pytest.mark.parametrize("I", P.C_INTERVALS)
def test_slot_stores_sit_on_every_boundary(I):
    off = P.slot_offsets(I)
    k = np.arange(1, P.HOUR // I)
    assert {0, P.HOUR - 1} <= set(off.tolist())
    assert set(np.concatenate([k * I - 1, k * I, k * I + 1]).tolist()) <= set(off.tolist())
    case = P.slot_case(I)
    dec = P.decode(case.store)
    second = np.concatenate([rows[1][1] - rows[1][0] * 1000 for rows in dec])
    assert sorted(second.tolist()) == off.tolist()
    assert all(len(r[1]) <= P.CH for rows in dec for r in rows)
    assert P.HOUR % I == 0
    assert I in (1000, 45000, 60000, 1800000) or float(np.float32(1.0) / np.float32(I)) * I != 1.0


@pytest.mark.parametrize("I", P.C_INTERVALS)
def test_float_quotient_is_exact_below_the_hour(I):
    """decode_row estimates off / I as (uint32)((float)off * (float)(1.0 / I)) and then corrects
    the quotient by up to -1 / +2.  Restated in IEEE single precision: for these intervals (and,
    scanned once, for every divisor of the hour) the estimate already is the quotient at every
    offset below the hour -- an offset is exact in float, and the relative error of the product,
    about 2^-23, is below the 1 / off that separates k I - 1 from k I.  So no store can tell a
    removed correction from the kernel; what the slot stores pin is the estimate itself (an
    estimate that rounds up, with the first correction removed, fails every one of them)."""
    off = np.arange(0, P.HOUR, dtype=np.int64)
    est = (off.astype(np.float32) * np.float32(1.0 / I)).astype(np.uint32).astype(np.int64)
    np.testing.assert_array_equal(est, off // I)


# ---- the restatement against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.CASES))
def test_restatement_equals_oracle(prepared, name):
    case, _prep = prepared(name)
    mine = P.restate(case.store, case.win, case.I)
    raised = 0
    for fn in P.FUNCS:
        try:
            want = O.run_query(case.store, P.query(case, fn))
        except O.OracleError as e:
            # an infinity that reaches an output: only the stores built for it
            assert e.java == "IllegalStateException" and name in P.E_INF_CASES, (fn, e)
            assert any(np.isinf(b.view(np.float64)).any() for _g, _t, b, _i in mine[fn]), fn
            raised += 1
            continue
        assert not any(np.isinf(b.view(np.float64)).any() for _g, _t, b, _i in mine[fn]), fn
        assert len(mine[fn]) == len(want), fn
        for (g1, t1, b1, i1), (g2, t2, b2, i2) in zip(mine[fn], want):
            assert g1 == g2, fn
            np.testing.assert_array_equal(t1, t2, err_msg=f"{fn} series {g1}: timestamps")
            np.testing.assert_array_equal(i1, i2)
            n1, n2 = np.isnan(b1.view(np.float64)), np.isnan(b2.view(np.float64))
            np.testing.assert_array_equal(n1, n2, err_msg=f"{fn} series {g1}: NaN positions")
            np.testing.assert_array_equal(b1[~n1], b2[~n2], err_msg=f"{fn} series {g1}: bits")
    if name in P.E_INF_CASES:
        assert raised < len(P.FUNCS)


def test_zero_stores_put_both_zeros_and_nan_on_the_ranks():
    for f64 in (False, True):
        case = P.zeros_case(f64)
        mine = P.restate(case.store, case.win, case.I, fns=("p999", "p99", "p90", "median"))
        for fn, groups in mine.items():
            bits = np.concatenate([b for _g, _t, b, _i in groups])
            assert (bits == 0x8000000000000000).sum() >= 4 and (bits == 0).sum() >= 4, fn
        assert np.isnan(np.concatenate([b for _g, _t, b, _i in mine["p999"]]).view(np.float64)).sum() >= 2   # Inf - Inf


# ---- the predictor, by hand -----------------------------------------------------------------------------------
def _hand_case():
    rng = np.random.default_rng(1)
    sizes = [(10, 100, 239), (10, 240), (239,), (512, 3)]
    parts = [P._rank_series(2, "f4", sz, rng, True) for sz in sizes]
    return P._case_of("hand", parts, (P.T0, P.T0 + 3 * 3600 - 1), P.HOUR, [(2, 4)] * 4)


def test_predict_p90_without_the_key_kernel():
    """PCT_KEYS off: the extraction kernel (variant 0) hands back exactly the series with a bucket of
    at least 240 values, whose p90 lies 25 from the top; with it on, the near-end key kernel does."""
    case = _hand_case()
    r = P.predict(case.store, case.win, case.I, "p90", {"PCT_KEYS": 0})
    assert (r.launched, r.variant) == (1, 0)
    assert r.back == {1: "a statistic more than 24 from both ends", 3: "a statistic more than 24 from both ends"}
    assert r.big == set() and r.waves == 0
    r = P.predict(case.store, case.win, case.I, "p90")
    assert (r.launched, r.variant, sorted(r.back)) == (1, 5, [1, 3])          # (a 512 row: 8 values a lane)
    r = P.predict(case.store, case.win, case.I, "p95")
    assert sorted(r.back) == [3]                                               # 512 > 479
    r = P.predict(case.store, case.win, case.I, "p50")
    assert (r.launched, r.variant, r.back) == (1, 6, {})                       # the rank search takes any rank
    r = P.predict(case.store, case.win, case.I, "p50", {"PCT_KEYS": 0})
    assert (r.launched, r.variant) == (0, -1)
    r = P.predict(case.store, case.win, case.I, "p99", {"PCT_ROWS": 0})
    assert r.readout() == (0, -1, 0, 0, 0)


def test_predict_six_or_eight_values_a_lane(prepared):
    for name, near, mid in (("q2f4_384", 13, 14), ("q4f4_384", 13, 14), ("q2f4_385", 5, 6), ("q2f4", 5, 6), ("q4i4", 5, 6),
                            ("mixed4", 1, 2), ("q2f8", 0, None), ("q4i1", 0, None)):
        case, prep = prepared(name)
        assert P.predict(case.store, case.win, case.I, "p99", prep=prep).variant == near, name
        r = P.predict(case.store, case.win, case.I, "median", prep=prep)
        assert (r.launched, r.variant) == ((1, mid) if mid else (0, -1)), name
    case, prep = prepared("q2f4_384")
    assert P.predict(case.store, case.win, case.I, "p99", {"PCT_V6": 0}, prep).variant == 5
    assert P.predict(case.store, case.win, case.I, "p75", {"PCT_VONLY": 0}, prep).variant == 2
    assert P.predict(case.store, case.win, case.I, "p999", {"PCT_KEYS": 0}, prep).variant == 0


def test_predict_hand_backs_by_value(prepared):
    case, prep = prepared("q2i4")
    r = P.predict(case.store, case.win, case.I, "p99", prep=prep)
    assert r.back == {4: "an INT32_MIN value"}
    r = P.predict(case.store, case.win, case.I, "p99", {"PCT_KEYS": 0}, prep)
    assert r.back == {}                                       # (the extraction reads doubles: INT32_MIN is a value like any)
    case, prep = prepared("mixed4")
    r = P.predict(case.store, case.win, case.I, "median", prep=prep)
    assert r.back == {0: "a row of mixed kinds", 1: "a row of mixed kinds"}
    case, prep = prepared("q2f8")
    r = P.predict(case.store, case.win, case.I, "p90", prep=prep)
    assert sorted(r.back) == [0, 1, 2, 3] and r.big == set()


@pytest.mark.parametrize("n1s", P.D_N1S)
def test_predict_chain(n1s):
    case, names = P.chain_case(n1s)
    r = P.predict(case.store, case.win, case.I, "p99")
    back = {names[s]: why for s, why in r.back.items()}
    # (two_cells stays: its two cells of one base time are one row once loaded)
    want = {"ms4097": "a row of another class", "past_hour": "an offset past the hour"}
    want.update({f"sec_{j}": "a row of more than 512 datapoints" for j in range(n1s)})
    assert back == want
    assert {names[s] for s in r.big} == {"ms4097"} | {f"sec_{j}" for j in range(n1s)}
    assert (r.launched, r.variant) == (1, 13)
    assert r.waves == {0: 2, 1: 2, 2: 4, 3: 4}[n1s]
    assert r.cap_min == (10800 if n1s else 4097)
    assert P.predict(case.store, case.win, case.I, "median").variant == 14


def test_predict_sizes_and_slots(prepared):
    case, prep = prepared("sizes")
    r = P.predict(case.store, case.win, case.I, "p99", prep=prep)
    assert r.readout() == (0, -1, 0, 7, 8) and r.cap_min == sum(P.SIZES)      # 3 h does not divide the hour
    case, prep = prepared("slots_1125")
    assert P.predict(case.store, case.win, case.I, "p90", prep=prep).readout() == (1, 0, 0, 0, 0)
    assert P.predict(case.store, case.win, case.I, "p75", prep=prep).readout() == (0, -1, 0, 0, 0)
