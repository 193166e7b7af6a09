"""The stores of the raw-path and group-by LERP edge tests are what they claim to be, and the
plain Python restatement of the raw path (tests/raw_edges.py: AggregationIterator, the
aggregators, the percentile estimate, RateSpan) equals the C oracle on every store and query of
tests/test_gpu_raw_edges.py, in bits and in exception.  No GPU."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import raw_edges as R
from tests import value_edges as V
from tests.test_lerp_window_math import java_lerp, lerpw


def oracle_outcome(batch, q):
    try:
        return O.run_query(batch, q), None
    except O.OracleError as e:
        return None, e.java


def assert_ref_is_oracle(store, q, ctx):
    want, ref = oracle_outcome(store.batch, q), R.ref_outcome(store, q)
    assert ref[1] == want[1], f"{ctx}: the Python reference raised {ref[1]}, the oracle {want[1]}"
    if want[1] is None:
        V.assert_bits(ref[0], want[0], ctx)
    return want


@pytest.fixture(scope="module")
def stores():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = (R.RAW_CASES.get(name) or R.PCT_CASES[name])[0]()
        return cache[name]
    return get


# ---- 0. the Python reference against the oracle ---------------------------------------------------
@pytest.mark.parametrize("name", list(R.RAW_CASES))
def test_reference_equals_oracle(stores, name):
    st = stores(name)
    assert st.n_points <= 150000
    for label, q in R.queries_of(name):
        assert_ref_is_oracle(st, q, f"{name} {label}")


@pytest.mark.parametrize("name", list(R.PCT_CASES))
def test_reference_equals_oracle_percentiles(stores, name):
    st = stores(name)
    for label, q in R.pct_queries_of(name):
        assert_ref_is_oracle(st, q, f"{name} {label}")


# ---- A.1 the guards of the strip-wide LERP ----------------------------------------------------------
def test_windows_sit_on_both_sides_of_every_guard():
    """Per den: windows the strip-wide path takes (ok) and windows it declines, dy on both sides
    of floor(2^50 / den), of floor(2^51 / den) and of 2^51, exact multiples of den of both signs;
    and where ok, the restated lerpw equals Java's long LERP at every evaluated point."""
    for den in R.WINDOW_DENS:
        dys = R.window_dys(den)
        oks = {dy: lerpw(1, 0, -7, den, -7 + dy) is not None for dy in dys}
        assert any(oks.values()) and not all(oks.values()), den
        for top in (50, 51):
            f = (1 << top) // den
            assert {f - 1, f, f + 1, -f + 1, -f, -f - 1} <= set(dys)
        assert {(1 << 51) - 1, 1 << 51, (1 << 51) + 1, -(1 << 51) + 1, -(1 << 51), -(1 << 51) - 1} <= set(dys)
        assert not oks[1 << 51] and not oks[(1 << 51) + 1] and not oks[-(1 << 51)]
        assert oks[(1 << 50) // den - 1] and not oks[(1 << 51) // den + 1]
        assert any(dy % den == 0 and dy > 0 and oks[dy] for dy in dys) and any(dy % den == 0 and dy < 0 and oks[dy] for dy in dys)
        assert any(dy % den == 1 and oks[dy] for dy in dys) and any(dy % den == den - 1 and oks[dy] for dy in dys)
        inner = [t - R.WIN_X0 for t in R.window_clock(den) if R.WIN_X0 < t < R.WIN_X0 + den]
        assert {1, den // 2, den - 1} - {0} <= set(inner)
        for dy in dys:
            if oks[dy]:
                for dx in inner:
                    assert lerpw(dx, 0, -7, den, -7 + dy) == java_lerp(dx, 0, -7, den, -7 + dy), (den, dy, dx)


def test_windows_reach_the_correction_branches():
    """The evaluated points of the ok windows take the two corrections that raise |q|: r >= den
    (dy > 0) and r <= -den (dy < 0) -- the quotient by the rounded reciprocal fell one short.

    The other two, r < 0 (dy > 0) and r > 0 (dy < 0), would lower |q|; under the guard they are
    unreachable.  The true quotient is t = n / den with the exact integer n = |x - x0| |dy| < 2^51
    (the guard bounds the rounded product |dy| den by 2^50, so the exact one by 2^51, and x - x0 <
    den).  The computed one is t (1 + e1)(1 + e2) with |e| <= 2^-53 (the rounding of 1 / den and of
    the product), so it exceeds t by less than t 2^-52 < 2^51 / den 2^-52 = 1 / (2 den).  For
    trunc() of it to exceed trunc(t), t would have to lie within that distance below an integer;
    but n is an integer, so a t that is no integer lies at least 1 / den below the next one.  Hence
    trunc(computed) <= trunc(t) always: the test asserts that no point of the set takes them."""
    seen = set()
    for den in R.WINDOW_DENS:
        inner = [t - R.WIN_X0 for t in R.window_clock(den) if R.WIN_X0 < t < R.WIN_X0 + den]
        for dy in R.window_dys(den):
            if lerpw(1, 0, -7, den, -7 + dy) is not None:
                seen |= {R.lerpw_branch(dx, den, dy) for dx in inner}
    assert {"r>=den", "r<=-den", "none"} <= seen, seen
    assert not seen & {"r<0", "r>0"}, seen


@pytest.mark.parametrize("den", [d for d in R.WINDOW_DENS if d >= 1000])
def test_window_strips(stores, den):
    """The window's first point has rank 511 (the last of strip 0), strip 1 (ranks 512..1023) lies
    strictly inside the window (m == 0), and its last point lies in strip 2 (m > 0)."""
    st = stores(f"window/{den}")
    u = R.union_of(st, 0, R.WIN2)
    assert u.index(R.WIN_X0) == R.STRIP - 1
    assert 2 * R.STRIP <= u.index(R.WIN_X0 + den) < 3 * R.STRIP
    assert all(R.WIN_X0 < t < R.WIN_X0 + den for t in u[R.STRIP:2 * R.STRIP])


def test_window_guard_at_2_32_ms():
    """den = 2^32 - 1 ms is the widest window the strip-wide path takes, 2^32 ms the first it
    declines (with dy small enough for the product guard).  Such a window spans 49.7 days of hour
    rows, so this edge is left to the arithmetic here: the restated lerpw against Java's LERP."""
    for dy in (1, -1, 262143, -262143, 1 << 17, -(1 << 17) - 1):
        for dx in (1, (1 << 31), (1 << 32) - 2):
            got = lerpw(dx, 0, 5, (1 << 32) - 1, 5 + dy)
            assert got is not None and got == java_lerp(dx, 0, 5, (1 << 32) - 1, 5 + dy)
        assert lerpw(1, 0, 5, 1 << 32, 5 + dy) is None
    assert lerpw(1, 0, 5, (1 << 32) - 1, 5 + 262144) is not None and lerpw(1, 0, 5, (1 << 32) - 1, 5 + 262145) is None   # the product passes 2^50


def test_jdiv_products():
    """(x - x0) dy of both signs at 2^53 - 1, 2^53 and 2^53 + 1; wrapped products with y0 at the
    ends of the long range.  den < 2^53 always holds: a timestamp has 44 bits at most."""
    prods = {dx * dy for dx, dy in R.JDIV_PRODUCTS}
    assert {(1 << 53) - 1, 1 << 53, (1 << 53) + 1} <= prods
    wraps = set()
    for y0, y1 in R.JDIV_WRAPS:
        dy = R.w64(y1 - y0)
        for dx in (3, 5, 4001):
            wraps.add(abs((dx * dy + (1 << 63)) >> 64))   # the multiples of 2^64 the wrapped product is off by
    assert {0, 1, 2} <= wraps
    assert any(y0 in (R.LONG_MAX, R.LONG_MIN) for y0, _ in R.JDIV_WRAPS)


# ---- A.4 values and exceptions per family ------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in R.RAW_CASES if n.startswith(("double/", "rate"))])
def test_families_return_values_and_raise(stores, name):
    """From the oracle alone: every family has a query that returns values, and every family that
    can hand an infinity to an aggregator (float64 cells; a float32 cell cannot overflow a double)
    has one that raises IllegalStateException."""
    st = stores(name)
    errs = {oracle_outcome(st.batch, q)[1] for _, q in R.queries_of(name)}
    assert None in errs, name
    fam = name.split("/")[1] if "/" in name else name
    if (fam in R.INF_FAMILIES and (fam == "inf" or name.endswith("f64"))) or name == "rate_inf":
        assert "IllegalStateException" in errs, name
    assert errs <= {None, "IllegalStateException"}, errs


def test_late_float_makes_early_points_double(stores):
    st = stores("double/late_float")
    (_, ts, _, is_int), _ = O.run_query(st.batch, R.abi.new_query(*R.WIN1, "sum"))
    nxt = R.M0 + 1700 * R.S   # the float point stays the span's current one until its next point is reached
    assert (ts < R.M0 + 1500 * R.S).sum() > 128
    assert not is_int[ts < nxt].any() and is_int[ts >= nxt].all() and (ts >= nxt).any()


# ---- A.6 strip geometry ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [R.LONG, R.F64])
@pytest.mark.parametrize("U", R.STRIP_SIZES)
def test_strip_ranks(U, kind):
    st = R.strip_store(U, kind)
    u = R.union_of(st, 0, R.WIN1)
    assert len(u) == U
    ranks = [[u.index(t) for t, _, _ in pts if t in u] for pts in st.series]
    b = R.strip_boundary(U)
    assert ranks[0] == list(range(U))
    if b:
        assert ranks[1] == [b - 1, b] and ranks[2][-1] == b - 1 and ranks[3][0] == b
        assert ranks[4] == [1, U - 2]
    assert [0] in ranks and [U - 1] in ranks and ranks[-1] == []
    if U > 512:
        assert b == 512


# ---- B. the overflowing LERP under a percentile ------------------------------------------------------------
def test_pct_overflow_oracle_is_finite_and_depends_on_the_infinity(stores):
    """p99 of the + case is finite in the oracle (and in the Python reference), p999 raises; without
    span A's +Inf operand the ranks shift by one and p99 differs.  The - case returns values."""
    st = stores("pct_overflow/+")
    q99, q999 = R.abi.new_query(*R.WIN1, "p99"), R.abi.new_query(*R.WIN1, "p999")
    want = assert_ref_is_oracle(st, q99, "pct_overflow/+ p99")
    assert want[1] is None
    vals = np.asarray(want[0][0][2]).view(np.float64)
    assert np.isfinite(vals).all() and len(vals) == 1800
    assert oracle_outcome(st.batch, q999)[1] == "IllegalStateException"
    ops = sorted(1e306 * (1 + 1e-9 * j) for j in range(299))
    with_inf = R.percentile(ops + [R.INF], 99.0, "legacy")
    pruned = R.percentile([-1.0] + ops, 99.0, "legacy")   # A counted, but with an operand below the rest
    ts = np.asarray(want[0][0][1])
    # (x - x0) 1e305 is infinite from 1.8 s after A's first point; at its last point A's operand is 1e305
    after = (ts > R.M0 + 92 * R.S) & (ts < R.M0 + 3540 * R.S)
    assert after.sum() == 1723 and (ts < R.M0 + 92 * R.S).sum() < 512 and (ts >= R.M0 + 3540 * R.S).sum() < 256 and with_inf != pruned and (vals[after] == with_inf).all()
    neg = stores("pct_overflow/-")
    for agg in ("p99", "p999", "p50"):
        assert oracle_outcome(neg.batch, R.abi.new_query(*R.WIN1, agg))[1] is None


# ---- C. missing buckets -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.sparse_stores()))
def test_sparse_stores_have_interpolated_and_absent_slots(name):
    make, win = R.sparse_stores()[name]
    st = make()
    assert st.n_points <= 150000
    interp, absent = R.slot_facts(st)
    assert interp > 0 and absent > 0, (name, interp, absent)
    for g in set(st.gids):
        mem = [i for i, x in enumerate(st.gids) if x == g]
        facts = R.slot_facts(V.Store([st.series[i] for i in mem], [0] * len(mem)))
        assert facts[0] > 0 and facts[1] > 0, (name, g, facts)
