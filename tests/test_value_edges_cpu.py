"""The value-edge stores are what they claim to be, before any GPU sees them (no device needed).

* the "may differ" stores of the certificate tests really have buckets whose sum depends on the
  order (a pairwise tree and the reversed order give other bits than Java's order), and the
  oracle returns Java's order;
* the "exact" stores add to the same bits in every order tried;
* cert_truth is checked against brute force over real doubles, its rule in a small format;
* tests/index_ref.py evaluates rows whose certificate threshold 2^(52 + lsb) is beyond a double.
"""
from __future__ import annotations

import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

from opentsdb_amd import abi
from oracle import oracle as O
from tests import index_ref as IR
from tests import value_edges as V


def oracle_buckets(store, interval, win, fn="sum"):
    """Per series: {bucket ts: value bits} of the oracle's downsampling (group-by none)."""
    q = abi.new_query(win[0], win[1], "none", ds_function=abi.AGG[fn], ds_interval_ms=interval)
    res = O.run_query(store.batch, q)
    assert len(res) == len(store.series)
    return [dict(zip((int(t) for t in ts), (int(b) for b in np.asarray(bits).view(np.uint64)))) for _, ts, bits, _ in res]


def orders(vals, seed):
    rng = np.random.default_rng(seed)
    yield V.tree_sum(vals)
    yield V.seq_sum(vals[::-1])
    for _ in range(20):
        yield V.seq_sum(rng.permutation(vals))


@pytest.mark.parametrize("name", list(V.CERT_MAY_DIFFER))
def test_may_differ_stores_depend_on_the_order(name):
    make, interval, win = V.CERT_MAY_DIFFER[name]
    st = make()
    assert st.n_points <= 150_000
    assert V.series_truth(st, interval) == "may_differ"
    want = oracle_buckets(st, interval, win)
    tree_differs = rev_differs = checked = 0
    for (ts, v, _), ob in zip(st.series, want):
        for t, vals in V.buckets_of(ts, v, interval).items():
            seq = V.bits_of(V.seq_sum(vals))
            tree_differs += V.bits_of(V.tree_sum(vals)) != seq
            rev_differs += V.bits_of(V.seq_sum(vals[::-1])) != seq
            if t in ob:
                assert ob[t] == seq, f"{name}: the oracle's bucket {t} is not the sequential sum"
                checked += 1
    assert checked and tree_differs >= 1 and rev_differs >= 1, (name, checked, tree_differs, rev_differs)


@pytest.mark.parametrize("name", list(V.CERT_EXACT))
def test_exact_stores_add_alike_in_every_order(name):
    make, interval, win = V.CERT_EXACT[name]
    st = make()
    assert V.series_truth(st, interval) in ("exact", "must_take_fast")
    want = oracle_buckets(st, interval, win)
    checked = 0
    for si, ((ts, v, _), ob) in enumerate(zip(st.series, want)):
        for t, vals in V.buckets_of(ts, v, interval).items():
            seq = V.bits_of(V.seq_sum(vals))
            for other in orders(np.asarray(vals), seed=si):
                assert V.bits_of(other) == seq, f"{name}: bucket {t} depends on the order"
            if t in ob:
                assert ob[t] == seq
                checked += 1
    assert checked


def test_boundary_stores_sit_where_they_claim():
    """(a): 60-point buckets of odd integers under 2^e -- 45 inside the documented threshold by a
    factor of two, 46 / 47 in the band around it, 48 past what the truth promises."""
    got = {e: V.series_truth(V.odd_ints_store(e, "one_row", n_series=2), 600000) for e in (45, 46, 47, 48)}
    assert got == {45: "must_take_fast", 46: "exact", 47: "exact", 48: "may_differ"}
    got = {m: V.series_truth(V.f32_mixed_store("one_row", m=m, big_every=0, n_series=2), 600000) for m in (15, 16, 17, 18)}
    assert got == {15: "must_take_fast", 16: "exact", 17: "exact", 18: "may_differ"}
    got = {e: V.series_truth(V.odd_ints_store(e, "one_row", n_series=2), 600000, square=True) for e in V.SQ_E}
    assert got == V.SQ_E
    for name, (make, interval, _) in V.CERT_PAST.items():
        assert V.series_truth(make(), interval) == "may_differ", name


def test_squares_of_the_boundary_stores_are_exact():
    """squareSum at e <= 23: every square (under 2^46) and every sum of 60 of them is exact."""
    for e in (22, 23):
        st = V.odd_ints_store(e, "one_row", n_series=2)
        for ts, v, _ in st.series:
            for vals in V.buckets_of(ts, v, 600000).values():
                sq = np.asarray(vals) ** 2
                assert all(int(x) ** 2 == int(y) for x, y in zip(vals, sq))
                assert int(V.seq_sum(sq)) == sum(int(x) ** 2 for x in vals) == int(V.tree_sum(sq))


# ---- cert_truth against brute force in a toy format: p-bit significands, integers (lsb 0) -------
def _round(x: int, p: int) -> int:
    """x rounded to p significant bits, ties to even."""
    a = abs(x)
    sh = a.bit_length() - p
    if sh <= 0:
        return x
    lo = a & ((1 << sh) - 1)
    a >>= sh
    half = 1 << (sh - 1)
    if lo > half or (lo == half and (a & 1)):
        a += 1
    return (a << sh) * (1 if x >= 0 else -1)


def _toy_truth(n, amax, p):
    """cert_truth's rule with 2^53 replaced by 2^p (lsb 0, no overflow)."""
    return "exact" if n * amax <= (1 << p) else "may_differ"


@pytest.mark.parametrize("p", [3, 4])
def test_cert_rule_against_brute_force(p):
    """Every multiset of n <= 3 integers bounded by A, in every order, with p-bit rounding after
    each addition: where the rule says exact, all orders give the exact sum; and the rule is not
    vacuous -- some set past it does depend on the order."""
    witness = False
    for n in (2, 3):
        for amax in range(1, (1 << p) + 3):
            vals = range(-amax, amax + 1)
            for combo in itertools.combinations_with_replacement(vals, n):
                if any(_round(x, p) != x for x in combo):
                    continue   # not a value of the format
                sums = set()
                for perm in set(itertools.permutations(combo)):
                    s = 0
                    for x in perm:
                        s = _round(s + x, p)
                    sums.add(s)
                if _toy_truth(n, amax, p) == "exact":
                    assert sums == {sum(combo)}, (p, n, amax, combo, sums)
                elif len(sums) > 1:
                    witness = True
    assert witness


@pytest.mark.parametrize("lsb", [0, -30, -1074, 900, 968])
def test_cert_truth_against_brute_force_in_doubles(lsb):
    """V.cert_truth itself against real double additions: multisets of n <= 3 multiples of 2^lsb
    around the threshold 2^(53 + lsb) / n and around zero, summed in every order.  Where cert_truth
    does not say "may_differ" every order gives the exact sum; past it some multiset of each n
    depends on the order or rounds."""
    u = Fraction(2) ** lsb
    witness = set()
    for n in (2, 3):
        top = (1 << 53) // n
        mags = sorted({1, 2, 3, top - 1, top, top + 1, top + 2, (1 << 52) - 1, 1 << 52, (1 << 52) + 1, (1 << 53) - 1, 1 << 53})
        vals = [float(m * u) for m in mags] + [-float(m * u) for m in mags]
        assert all(Fraction(v) / u == int(Fraction(v) / u) for v in vals)   # each a double, a multiple of 2^lsb
        for combo in itertools.combinations_with_replacement(vals, n):
            truth = V.cert_truth(n, lsb, max(abs(x) for x in combo))
            sums = set()
            for perm in set(itertools.permutations(combo)):
                acc = 0.0
                for x in perm:
                    acc += x
                sums.add(acc)
            if truth != "may_differ":
                exact = sum(Fraction(x) for x in combo)
                assert all(Fraction(x) == exact for x in sums), (n, lsb, combo, sums)
            elif len(sums) > 1 or any(Fraction(x) != sum(Fraction(y) for y in combo) for x in sums):
                witness.add(n)   # (two values commute: past the rule their one sum is inexact instead)
    assert witness == {2, 3}


def test_cert_truth_is_the_rule_at_53_bits():
    rng = np.random.default_rng(5)
    for _ in range(300):
        lsb = int(rng.integers(-1074, 960))
        n = int(rng.integers(1, 5000))
        odd = 2 * int(rng.integers(0, 1 << 52)) + 1
        amax = math.ldexp(float(odd), lsb) if odd.bit_length() + lsb <= 1023 else None
        if amax is None or amax == 0.0 or odd.bit_length() + lsb < -1000:
            continue
        # integers only: n * odd against 2^53, 2^51; overflow against 2^(1024 - lsb)
        exact = n * odd <= 1 << 53 and (lsb > 1024 or n * odd < 1 << (1024 - lsb))
        must = n * odd <= 1 << 51 and (lsb > 1023 or n * odd < 1 << (1023 - lsb))
        t = V.cert_truth(n, lsb, amax)
        assert t == ("must_take_fast" if must else "exact" if exact else "may_differ"), (n, lsb, odd)
    # the edges the formula in floating point gets wrong or cannot evaluate
    assert V.cert_truth(60, 1023, V.HUGE) == "may_differ"       # 60 * 2^1023 overflows
    assert V.cert_truth(2, 1023, V.HUGE) == "may_differ"        # 2^1024 is no double
    assert V.cert_truth(1, 1023, V.HUGE) == "exact"
    assert V.cert_truth(60, 1000, 2.0 ** 1000) == "must_take_fast"   # threshold 2^1052 is beyond a double
    assert V.cert_truth(1 << 20, 1003, 2.0 ** 1003) == "exact"       # 2^1023: below 2^1024, not below 2^1023
    assert V.cert_truth(4, -1074, 5e-324) == "must_take_fast"


def test_overflow_bucket_is_order_dependent_and_the_oracle_keeps_javas_order():
    st = V.overflow_store()
    ts, v, _ = st.series[0]
    for vals in V.buckets_of(ts, v, 600000).values():
        assert len(vals) == 60
        # Java's order: M + M = Inf; pairs first: Inf + -Inf = NaN; alternating signs: 0
        assert V.seq_sum(vals) == math.inf and math.isnan(V.tree_sum(vals))
        assert V.seq_sum([x for pair in zip(vals[0::4], vals[2::4]) for x in pair] * 2) == 0.0
    lsb, amax = V.facts_of(v)
    assert (lsb, amax) == (1023, V.HUGE) and V.cert_truth(60, lsb, amax) == "may_differ"
    q = abi.new_query(V.T0, V.T0 + 3599, "min", ds_function=abi.AGG["sum"], ds_interval_ms=600000)
    (_, _, bits, _), = O.run_query(st.batch, q)
    assert list(np.asarray(bits).view(np.float64)) == [60.0] * 6       # min(+Inf, 60 x 1.0)
    for agg in ("sum", "avg"):
        q = abi.new_query(V.T0, V.T0 + 3599, agg, ds_function=abi.AGG["sum"], ds_interval_ms=600000)
        with pytest.raises(O.OracleError) as e:
            O.run_query(V.overflow_store(partner=False).batch, q)
        assert e.value.java == "IllegalStateException"


def test_overflow_arrangements_are_order_dependent():
    """Of the +-2^1023 arrangements some overflow in Java's order and some do not; for each stride
    some bucket's sequential sum differs from its tree or reversed sum, and every series fails the
    certificate's truth."""
    for stride in V.OVERFLOW_STRIDES:
        inf = fin = differs = 0
        for pattern in V.OVERFLOW_PATTERNS:
            st = V.overflow_pattern_store(pattern, stride)
            ts, v, _ = st.series[0]
            lsb, amax = V.facts_of(v)
            assert (lsb, amax) == (1023, V.HUGE)
            for vals in V.buckets_of(ts, v, 600000).values():
                seq = V.seq_sum(vals)
                inf += math.isinf(seq)
                fin += math.isfinite(seq)
                n = sum(1 for x in vals if x)
                assert n >= 2 and V.cert_truth(len(vals), lsb, amax) == "may_differ"
                for other in (V.tree_sum(vals), V.seq_sum(vals[::-1])):
                    differs += not (other == seq)
        assert inf and fin and differs, (stride, inf, fin, differs)


# ---- the host row classifier past the double range ----------------------------------------------
def test_index_ref_evaluates_rows_whose_threshold_is_beyond_a_double():
    """52 + lsb > 1023: math.ldexp(1.0, 52 + lsb) raises; the certificate there turns on the
    overflow of n * absmax alone."""
    assert IR.row_nocert(1023, V.HUGE) is True              # 2 * 2^1023 overflows: M + M = Inf, (M + -M) + M = M
    assert IR.row_nocert(1000, 2.0 ** 1000) is False        # 2^1001, exact
    assert IR.row_nocert(972, math.ldexp(float((1 << 52) + 1), 971)) is True   # lsb 971: 52 + lsb = 1023, the last finite threshold
    assert IR.row_nocert(980, 2.0 ** 1022) is False         # 2^1023 finite, a multiple of 2^980 under 2^(53 + 980)
    assert IR.row_nocert(0, 2.0 ** 50) is False and IR.row_nocert(0, 2.0 ** 52) is True   # unchanged below
    assert IR.row_nocert(IR.INT32_MAX, math.inf) is False and IR.row_nocert(3, math.inf) is True
    for lsb, amax in ((1023, V.HUGE), (1000, 2.0 ** 1000), (980, 2.0 ** 1022), (0, 2.0 ** 52), (-30, 2.0 ** 30)):
        # the engine's threshold 2^(52 + lsb) is cert_truth's 2^(53 + lsb') at lsb' = lsb - 1
        assert IR.row_nocert(lsb, amax) == (V.cert_truth(2, lsb - 1, amax) == "may_differ"), (lsb, amax)
    st = V.overflow_store()
    ndp, flags, lsb, amax, facts = IR.index_ref(st.batch)
    assert facts[0].lsb == 1023 and facts[0].absmax == V.HUGE and facts[0].nocert
    assert flags[0] & IR.ROW_NOCERT and not flags[1] & IR.ROW_NOCERT


def test_scale_sweep_base_is_order_free_and_which_scales_are_pure_scalings():
    """(g): the dyadic base adds exactly in any order; 2^s x it is a pure scaling of the oracle's
    result exactly when nothing under- or overflows -- decided from the oracle alone.  Sums scale
    at every s (2^-1070 is still a subnormal's multiple); an average rounds anew among the subnormals."""
    ts, vals, _ = V.dyadic_base()
    for si, v in enumerate(vals):
        for b in V.buckets_of(ts, v, 600000).values():
            seq = V.bits_of(V.seq_sum(b))
            for other in orders(np.asarray(b), seed=si):
                assert V.bits_of(other) == seq
    # avg divides by 60 and diff subtracts two sums: both round anew among the subnormals
    impure_of = {"avg": {-1060}, "count": set(V.SCALES_F64) - {0}}   # (a count is a float here and does not scale)
    for fn in ("sum", "avg", "min", "max", "count", "first", "last", "diff"):
        for level in ("ds", "group"):
            agg, ds = ("none", fn) if level == "ds" else (fn, "sum")
            q = abi.new_query(V.T0, V.T0 + 3599, agg, ds_function=abi.AGG[ds], ds_interval_ms=600000)
            base = O.run_query(V.scaled_store(0).batch, q)
            impure = {s for s in V.SCALES_F64 if not V.is_pure_scaling(base, O.run_query(V.scaled_store(s).batch, q), s)}
            assert impure == impure_of.get(fn, set()), (fn, level, impure)
