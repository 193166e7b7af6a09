"""GPU parity of tsdbhip_upsert (k_upsert.hip): rows upserted by (series, base time) anywhere in
the resident batch without a reload.

The expectation never comes from the engine: after load(A) + upsert(D) the context must answer
as a fresh load of merge_batches(A, D) would (tests/append_util.py, checked against stores built
from full point lists for deltas that are not tail-shaped in tests/test_upsert_cpu.py).  Every
case follows tests/test_gpu_append.py's check_append: it first queries the OLD state, upserts,
compares every query with the oracle over the merged batch restricted to its visible series bit
for bit (tol = 0.0), and then compares results, debug_rows(), download(), sizes, the resident
group order and debug_regular()'s array with the same engine after a fresh load of that batch.

Inputs are order-free -- integers, or multiples of 0.25 below 2^20 -- and every series has a
point in every bucket between its first and last point once the delta is in, so that no LERP
fraction enters a sum; `dev` and full-mantissa floats run under TSDB_QF_ORDERED."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import pytest

from opentsdb_amd import abi, synth
from oracle import oracle as O
from tests.append_util import Points, batches_equal, int_points, merge_batches, quarter_points, split, with_ids
from tests.test_gpu_append import same_state, sec_row, sizes, small_store, state
from tests.test_gpu_parity import assert_groups_match
from tests.test_gpu_preagg import FUNCS, resident_cells
from tests.test_gpu_regroup import agg_name, dsq, identical, resident_order, restricted, want_of
from tests.test_upsert_cpu import POSITIONS, position_case, replaced_rows, upsert_case, without

gpu = pytest.mark.gpu

T0 = 1356998400
H = 3600
EXCL = abi.GROUP_EXCLUDED
NONE = abi.GROUP_NONE
UNSORTED = 0x100000
al = lambda x: (int(x) + 15) & ~15   # noqa: E731


@pytest.fixture(scope="module")
def eng():
    from opentsdb_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def check_upsert(eng, a, d, idx, new, queries, ctx, loaded=False, old_queries=None, full=None):
    """One case.  `a` carries the PRESENT ids of the resident series (GROUP_EXCLUDED included,
    when the caller has regrouped).  Returns (info, results, merged batch)."""
    if not loaded:
        eng.load(a)
    for q in (queries if old_queries is None else old_queries):
        eng.run(q)                                   # the old state
    info = eng.upsert(d, idx, new)
    m = merge_batches(a, d, idx, new)
    if full is not None:
        batches_equal(m, full)
    rb, kept = restricted(m, m.group_id)
    assert eng.n_series() == len(kept), ctx
    got = state(eng, queries)
    reg = eng.debug_regular()[0]
    for i, (q, g) in enumerate(zip(queries, got[0])):
        assert_groups_match(g, want_of(rb, q), agg_name(q), tol=0.0, ctx=f"{ctx} q{i} vs oracle")
    np.testing.assert_array_equal(got[4], resident_order(rb.group_id))
    assert got[3] == (rb.n_series, rb.n_rows, int(rb.row_qual_off[-1]), int(rb.row_val_off[-1])), ctx
    rep = replaced_rows(a, d, idx, new)
    assert (info.series_added, info.rows_added, info.rows_replaced) == (int(np.count_nonzero(new)), d.n_rows - rep, rep), ctx
    eng.load(rb)
    same_state(got, state(eng, queries), queries, ctx)
    np.testing.assert_array_equal(reg, eng.debug_regular()[0], err_msg=f"{ctx} debug_regular")
    return info, got[0], m


def std_queries(lo, hi):
    return [dsq(lo, hi, "sum", "sum", 60000), dsq(lo, hi, "max", "max", 60000), abi.new_query(lo, hi - 1, "sum")]


# ---- 1. positions -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", POSITIONS)
def test_positions(eng, name):
    a, d, idx, new, full = upsert_case(*position_case(name))
    info, got, _ = check_upsert(eng, a, d, idx, new, std_queries(T0, T0 + 4 * H), name, full=full)
    assert len(got[0]) == 3 and info.rows_reindexed == 0
    if name == "before_first":
        assert (info.rows_added, info.rows_replaced) == (4, 0)
    if name == "replace_all":
        assert (info.rows_added, info.rows_replaced) == (0, 16)
    if name == "mixed":
        assert (info.series_added, info.rows_added, info.rows_replaced) == (1, 1 + 4 + 4 + 1, 1 + 1 + 1)


@gpu
def test_worked_example_and_a_single_series(eng):
    """Resident hours {0, 1, 2, 4} and delta hours {1, 3, 4} of one series: lb = {1, 3, 3}, hit =
    {1, 0, 1}, dest = {1, 3, 4} -- R0, D0, R2, D1, D2 (hits and misses interleaved); the same in a
    store of that one series only."""
    rng = np.random.default_rng(17)
    ts = T0 + np.arange(0, 5 * H, 60)
    pts = [int_points(rng, ts, -100, 30000) for _ in range(3)]
    half = lambda b: (b + 1800, b + H)   # noqa: E731
    late = [(T0 + 3 * H, T0 + 4 * H), half(T0 + H), half(T0 + 4 * H)]
    hours = [T0 + H, T0 + 3 * H, T0 + 4 * H]
    qs = std_queries(T0, T0 + 5 * H)
    a, d, idx, new, full = upsert_case(pts, [0, 0, 1], [[], late, []], [None, hours, None])
    assert a.n_rows == 5 + 4 + 5
    info, _, _ = check_upsert(eng, a, d, idx, new, qs, "worked example", full=full)
    assert (info.rows_added, info.rows_replaced) == (1, 2)
    a, d, idx, new, full = upsert_case(pts[1:2], [0], [late], [hours])
    info, _, _ = check_upsert(eng, a, d, idx, new, qs, "one series", full=full)
    assert (info.rows_added, info.rows_replaced) == (1, 2)


@gpu
def test_duplicated_series_base_in_the_delta(eng):
    """Two delta rows of one (series, base), out of base order with a third: merged first, as a
    load merges them."""
    rng = np.random.default_rng(23)
    ts = T0 + np.arange(0, 3 * H, 60)
    pts = [int_points(rng, ts, -100, 30000) for _ in range(4)]
    gids = [0, 1, 0, 1]
    a = synth.from_series([without(p, [(T0 + H, T0 + 2 * H), (T0 + 1800, T0 + H)]).rows() if s in (0, 2) else p.rows()
                           for s, p in enumerate(pts)], gids)
    # hour 1 in two rows of base T0 + H (its halves), the rewritten hour 0 between them
    d = synth.from_series([pts[s].rows(T0 + H, T0 + H + 1800) + pts[s].rows(T0, T0 + H) + pts[s].rows(T0 + H + 1800, T0 + 2 * H)
                           for s in (0, 2)], [0, 0])
    full = synth.from_series([p.rows() for p in pts], gids)
    qs = std_queries(T0, T0 + 3 * H)
    eng.load(a)
    info = eng.upsert(d, [0, 2], [0, 0])
    assert (info.rows_added, info.rows_replaced) == (2, 2)
    got = state(eng, qs)
    for i, (q, g) in enumerate(zip(qs, got[0])):
        assert_groups_match(g, O.run_query(full, q), agg_name(q), tol=0.0, ctx=f"duplicated q{i}")
    assert got[3][:2] == (4, 12)
    eng.load(merge_batches(a, d, [0, 2], [0, 0]))
    same_state(got, state(eng, qs), qs, "duplicated (series, base)")


# ---- 2. tail shape ------------------------------------------------------------------------------
@gpu
def test_tail_shape_equals_append(eng):
    rng = np.random.default_rng(29)
    n = 9
    pts = [quarter_points(rng, T0 + np.arange(0, 4 * H, 30)) if s % 2 else int_points(rng, T0 + np.arange(0, 4 * H, 30), -100, 30000)
           for s in range(n)]
    a, d, idx, new, full = split(pts, [s % 3 for s in range(n)], T0 + 2 * H + 1800, resident=[True] * 4 + [False] + [True] * 4)
    qs = std_queries(T0, T0 + 4 * H)
    eng.load(a)
    ia = eng.append(d, idx, new)
    sa = state(eng, qs)
    ra = eng.debug_regular()[0]
    eng.load(a)
    iu = eng.upsert(d, idx, new)
    same_state(state(eng, qs), sa, qs, "tail shape")
    np.testing.assert_array_equal(eng.debug_regular()[0], ra)
    assert (iu.series_added, iu.rows_added, iu.rows_replaced, iu.rows_reindexed) == (ia.series_added, ia.rows_added, ia.rows_replaced, 0)
    assert (iu.qual_dead, iu.val_dead, iu.qual_capacity, iu.val_capacity) == (ia.qual_dead, ia.val_dead, ia.qual_capacity, ia.val_capacity)


# ---- 3. row classes -----------------------------------------------------------------------------
@gpu
def test_backfill_turns_short_series_into_rows(eng):
    """One 360-point row a series (k_short) gains the hour before it."""
    rng = np.random.default_rng(31)
    pts = [quarter_points(rng, T0 + np.arange(0, 2 * H, 10)) if s % 2 else int_points(rng, T0 + np.arange(0, 2 * H, 10), -100, 30000)
           for s in range(12)]
    a, d, idx, new, full = upsert_case(pts, [s % 3 for s in range(12)], [[(T0, T0 + H)]] * 12, [[T0]] * 12)
    assert a.n_rows == 12
    qs = std_queries(T0, T0 + 2 * H) + [dsq(T0, T0 + 2 * H, "p99", "avg", 60000)]
    info, _, _ = check_upsert(eng, a, d, idx, new, qs, "short back-fill", full=full,
                              old_queries=std_queries(T0 + H, T0 + 2 * H))
    assert (info.rows_added, info.rows_replaced) == (12, 0)


@gpu
@pytest.mark.parametrize("opts", [{}, {"INDEX_FUSED": 0}, {"INDEX_GENERIC": 1}], ids=["default", "unfused", "generic"])
@pytest.mark.parametrize("kind", ["ms", "f64", "int16"])
def test_middle_row_replaced_by_another_class(eng, kind, opts):
    """A float32-only load (no int16 value copy): the middle hour's row is replaced by one with
    millisecond qualifiers, with float64 values, with 1-2-byte integers that need the copy."""
    from opentsdb_amd import engine
    rng = np.random.default_rng(37)
    n = 10
    gids = [s % 3 for s in range(n)]
    ts = T0 + np.arange(0, 3 * H, 10)
    mid = ts[(ts >= T0 + H) & (ts < T0 + 2 * H)]
    a = synth.from_series([quarter_points(rng, ts).rows() for _ in range(n)], gids)
    if kind == "ms":
        rows = [int_points(rng, mid, -1000, 1000, ms=True).rows() for _ in range(n)]
    elif kind == "f64":
        fv = lambda: rng.integers(1, 1 << 22, len(mid)).astype(np.float64) * 0.25   # noqa: E731
        rows = [Points(mid * 1000, fvals=fv(), kind=np.full(len(mid), 2)).rows() for _ in range(n)]
    else:
        rows = [int_points(rng, mid, -100, 30000).rows() for _ in range(n)]
    touched = [0, 2, 3, 5, 6, 9]
    d = synth.from_series([rows[s] for s in touched], [gids[s] for s in touched])
    with engine.options(**opts):
        info, _, _ = check_upsert(eng, a, d, np.array(touched), np.zeros(len(touched)), std_queries(T0, T0 + 3 * H),
                                  f"{kind} {opts}")
    assert (info.rows_added, info.rows_replaced) == (0, len(touched))


@gpu
def test_walker_row_replaced_in_the_middle(eng):
    """A 3000-point row in the middle of three-hour 1 s series replaced by the 3600-point one."""
    rng = np.random.default_rng(41)
    pts = [quarter_points(rng, T0 + np.arange(0, 3 * H, 1)) for _ in range(5)]
    a, d, idx, new, full = upsert_case(pts, [0, 1, 0, 1, 0], [[(T0 + H + 3000, T0 + 2 * H)]] * 5, [[T0 + H]] * 5)
    qs = [dsq(T0, T0 + 3 * H, "sum", "sum", 60000), dsq(T0, T0 + 3 * H, "max", "max", 60000)]
    info, _, _ = check_upsert(eng, a, d, idx, new, qs, "walker", full=full)
    assert (info.rows_added, info.rows_replaced) == (0, 5)


@gpu
def test_ordered_full_mantissa(eng):
    rng = np.random.default_rng(4)
    pts = [Points((T0 + np.arange(1080) * 10) * 1000, fvals=45.0 + 10.0 * rng.random(1080), kind=np.full(1080, 2))
           for _ in range(8)]
    a, d, idx, new, full = upsert_case(pts, [i % 2 for i in range(8)], [[(T0 + H + 900, T0 + 2 * H)]] * 8, [[T0 + H]] * 8)
    qs = [dsq(T0, T0 + 3 * H, "sum", "sum", 60000, flags=abi.QF_ORDERED), dsq(T0, T0 + 3 * H, "dev", "avg", 600000, flags=abi.QF_ORDERED)]
    check_upsert(eng, a, d, idx, new, qs, "ordered f64", full=full)


# ---- 4. flags -----------------------------------------------------------------------------------
def flag_rows():
    """(resident rows, delta rows) of five one-series groups; see test_flags."""
    res = [
        [sec_row(T0, [0, 600], [1, 2]), sec_row(T0 + 2 * H, [10, 20, 30], [3, 4, 5])],
        [sec_row(T0, [0, 600, 1200, 3700], [1, 2, 3, 4]), sec_row(T0 + H, [10, 20, 30], [9, 10, 11])],
        [sec_row(T0, [0, 3650], [1, 2]), sec_row(T0 + H, [5, 3700], [3, 4]), sec_row(T0 + 2 * H, [10, 50], [5, 6])],
        [sec_row(T0, [0, 900], [5, 6]), sec_row(T0 + H, [100, 40, 900], [14, 15, 16])],
        [sec_row(T0, [0, 900], [5, 6]), sec_row(T0 + 2 * H, [100, 40, 900], [14, 15, 16])],
    ]
    dlt = [
        [sec_row(T0 + H, [5, 3700], [21, 22])],              # inserted, reaches past the next row's first point
        [sec_row(T0, [0, 600, 1200, 3500], [1, 2, 3, 4])],   # the cause replaced by a row inside its hour
        [sec_row(T0, [0, 100], [1, 2])],                     # a cause replaced; the row between still reaches past the last
        [sec_row(T0, [0, 800], [5, 6])],                     # the later row is unsorted in itself
        [sec_row(T0 + H, [7, 60], [23, 24])],                # a pure insertion before a flagged row
    ]
    return res, dlt


@gpu
@pytest.mark.parametrize("opts", [{}, {"INDEX_FUSED": 0}, {"INDEX_GENERIC": 1}], ids=["default", "unfused", "generic"])
def test_flags(eng, opts):
    from opentsdb_amd import engine
    res, dlt = flag_rows()
    gids = [0, 1, 2, 3, 4]
    a = synth.from_series(res, gids)
    d = synth.from_series(dlt, gids)
    qs = [dsq(T0, T0 + 3 * H, "sum", "sum", 60000), abi.new_query(T0, T0 + 3 * H - 1, "sum")]
    flagged = lambda: [bool(f & UNSORTED) for f in eng.debug_rows()[1]]   # noqa: E731
    with engine.options(**opts):
        eng.load(a)
        assert flagged() == [False, False, False, True, False, True, True, False, True, False, True]
        assert eng.debug_regular()[0][3].tolist() == [0, 0]
        info, _, _ = check_upsert(eng, a, d, np.arange(5), np.zeros(5), qs, f"flags {opts}", loaded=True)
        # series 1's later row, series 2's two later rows, series 3's later row
        assert (info.rows_added, info.rows_replaced, info.rows_reindexed) == (2, 3, 4)
        eng.load(a)
        eng.upsert(d, np.arange(5), np.zeros(5))
        got = flagged()
        reg = eng.debug_regular()[0]
        # pure insertions only: no row is indexed again
        eng.load(a)
        info = eng.upsert(synth.from_series([dlt[0], dlt[4]], [0, 4]), [0, 4], [0, 0])
        assert (info.rows_added, info.rows_replaced, info.rows_reindexed) == (2, 0, 0)
        assert flagged() == [False, False, True, False, True, False, True, True, False, True, False, False, True]
    #              s0: R0   D     R2    s1: D  R1     s2: D  R1     R2    s3: D  R1    s4: R0  D      R2
    assert got == [False, False, True, False, False, False, False, True, False, True, False, False, True]
    assert reg[2].tolist()[1] == 0            # flagged by the inserted row: not regular any more
    assert reg[4].tolist() == [10, 10]        # the flag's cause is gone: the RegRow is back
    assert reg[7].tolist()[1] == 0 and reg[9].tolist()[1] == 0 and reg[12].tolist()[1] == 0


# ---- 5. with regroup ----------------------------------------------------------------------------
@gpu
def test_with_regroup(eng):
    rng = np.random.default_rng(13)
    n = 9
    pts = [quarter_points(rng, T0 + np.arange(0, 3 * H, 30)) for _ in range(n)]
    late = [[(T0 + H, T0 + 2 * H)] if s % 2 else [(T0 + 900, T0 + H)] for s in range(n)]
    hours = [[T0 + H] if s % 2 else [T0] for s in range(n)]
    a, d, idx, new, full = upsert_case(pts, [0] * n, late, hours, resident=[True] * 4 + [False] + [True] * 4)
    d = with_ids(d, np.where(new != 0, 2, 0))
    ids = np.array([1, EXCL, 0, 0, EXCL, 1, NONE, 0], np.int32)     # excluded and ungrouped series receive back-fill
    qs = [dsq(T0, T0 + 3 * H, "sum", "sum", 60000), dsq(T0, T0 + 3 * H, "none", "sum", 600000)]
    eng.load(a)
    eng.regroup(ids)
    _, got, m = check_upsert(eng, with_ids(a, ids), d, idx, new, qs, "after regroup", loaded=True)
    assert [g for g, *_ in got[0]] == [0, 1, 2]
    assert m.group_id.tolist() == [1, EXCL, 0, 0, 2, EXCL, 1, NONE, 0]
    # a later regroup, ids in the NEW index space, readmits the excluded series with their back-filled rows
    eng.load(a)
    eng.regroup(ids)
    eng.upsert(d, idx, new)
    ids2 = np.array([0, 1, EXCL, 0, 1, 1, 0, 0, NONE], np.int32)
    eng.regroup(ids2)
    got = state(eng, qs)
    rb, _ = restricted(full, ids2)
    for i, (q, g) in enumerate(zip(qs, got[0])):
        assert_groups_match(g, want_of(rb, q), agg_name(q), tol=0.0, ctx=f"readmitted q{i}")
    eng.load(rb)
    same_state(got, state(eng, qs), qs, "readmitted")


# ---- 6. growth and dead bytes -------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("reserve", [0, 50], ids=["exact", "fifty"])
def test_growth_and_dead_bytes(eng, reserve):
    from opentsdb_amd import engine
    rng = np.random.default_rng(21)
    n = 8
    pts = [quarter_points(rng, T0 + np.arange(0, 5 * H, 30)) for _ in range(n)]
    gids = [s % 2 for s in range(n)]
    qs = [dsq(T0, T0 + 5 * H, "sum", "sum", 60000), dsq(T0, T0 + 5 * H, "max", "max", 60000)]
    # hours 1 and 3 hold their first quarter only; each call rewrites one of them
    cur = synth.from_series([without(p, [(T0 + H + 900, T0 + 2 * H), (T0 + 3 * H + 900, T0 + 4 * H)]).rows() for p in pts], gids)
    with engine.options(APPEND_RESERVE=reserve):
        eng.load(cur)
        grew, dead_q, dead_v = [], 0, 0
        for b in (T0 + H, T0 + 3 * H):
            dd = synth.from_series([p.rows(b, b + H) for p in pts], gids)
            hit = cur.row_base_time[:cur.n_rows] == b
            dead_q += sum(al(x) for x in np.diff(cur.row_qual_off.astype(np.int64))[hit])
            dead_v += sum(al(x) for x in np.diff(cur.row_val_off.astype(np.int64))[hit])
            info = eng.upsert(dd, np.arange(n), np.zeros(n))
            cur = merge_batches(cur, dd, np.arange(n), np.zeros(n))
            grew.append(info.grew)
            assert (info.rows_added, info.rows_replaced) == (0, n)
            assert (info.qual_dead, info.val_dead) == (dead_q, dead_v), b
        got = state(eng, qs)
        assert grew == ([1, 1] if reserve == 0 else [1, 0])
        batches_equal(cur, synth.from_series([p.rows() for p in pts], gids))
        for i, (q, g) in enumerate(zip(qs, got[0])):
            assert_groups_match(g, O.run_query(cur, q), agg_name(q), tol=0.0, ctx=f"growth {reserve} q{i}")
        t = eng.trim(0, 0)                          # evicts nothing, packs: the dead bytes are reclaimed
        assert (t.rows_evicted, t.packed, t.qual_dead, t.val_dead) == (0, 1, 0, 0)
        assert t.qual_reclaimed >= dead_q and t.val_reclaimed >= dead_v
        packed = state(eng, qs)
    eng.load(cur)
    fresh = state(eng, qs)
    same_state(got, fresh, qs, f"growth {reserve}")
    same_state(packed, fresh, qs, f"growth {reserve} packed")


# ---- 7. sequence --------------------------------------------------------------------------------
@gpu
def test_sequence(eng):
    """load, append, upsert, trim(pack), upsert (a row below the trim cutoff included), regroup."""
    from tests.trim_util import trim_batch
    rng = np.random.default_rng(43)
    n = 8
    pts = [int_points(rng, T0 + np.arange(0, 5 * H, 60), -100, 30000) if s % 2 else quarter_points(rng, T0 + np.arange(0, 5 * H, 60))
           for s in range(n)]
    gids = [s % 2 for s in range(n)]
    ar = np.arange(n)
    z = np.zeros(n)
    # at the load: up to 3 h 30 min, hour 1's second half missing, hour 0 missing altogether
    old = [without(p, [(T0, T0 + H), (T0 + H + 1800, T0 + 2 * H)]) for p in pts]
    cur = synth.from_series([p.rows(None, T0 + 3 * H + 1800) for p in old], gids)
    eng.load(cur)
    d1 = synth.from_series([p.rows(T0 + 3 * H, T0 + 5 * H) for p in pts], gids)           # the tail
    eng.append(d1, ar, z)
    cur = merge_batches(cur, d1, ar, z)
    d2 = synth.from_series([p.rows(T0 + H, T0 + 2 * H) for p in pts], gids)               # hour 1 rewritten
    info = eng.upsert(d2, ar, z)
    assert (info.rows_added, info.rows_replaced) == (0, n)
    cur = merge_batches(cur, d2, ar, z)
    t = eng.trim(T0 + 2 * H, 0)
    assert (t.rows_evicted, t.packed, t.qual_dead) == (n, 1, 0)
    cur = trim_batch(cur, T0 + 2 * H)
    half = [0, 3, 4, 7]
    d3 = synth.from_series([pts[s].rows(T0, T0 + H) + pts[s].rows(T0 + 3 * H, T0 + 4 * H) for s in half], [gids[s] for s in half])
    info = eng.upsert(d3, half, np.zeros(4))                                             # hour 0 lies below the cutoff
    assert (info.rows_added, info.rows_replaced) == (4, 4)
    cur = merge_batches(cur, d3, half, np.zeros(4))
    ids = np.array([1, 0, EXCL, 0, 1, NONE, 0, 1], np.int32)
    eng.regroup(ids)
    qs = [dsq(T0 + 2 * H, T0 + 5 * H, "sum", "sum", 60000), dsq(T0 + 2 * H, T0 + 5 * H, "max", "max", 60000)]
    got = state(eng, qs)
    rb, _ = restricted(cur, ids)
    for i, (q, g) in enumerate(zip(qs, got[0])):
        assert_groups_match(g, want_of(rb, q), agg_name(q), tol=0.0, ctx=f"sequence q{i}")
    reg = eng.debug_regular()[0]
    eng.load(rb)
    same_state(got, state(eng, qs), qs, "sequence")
    np.testing.assert_array_equal(reg, eng.debug_regular()[0])


# ---- 8. malformed cell --------------------------------------------------------------------------
@gpu
def test_malformed_cell_inserted_mid_series(eng):
    from opentsdb_amd.engine import EngineError
    rng = np.random.default_rng(2)
    pts = [int_points(rng, T0 + np.arange(0, 3 * H, 60), 0, 100) for _ in range(3)]
    a = synth.from_series([without(p, [(T0 + H, T0 + 2 * H)]).rows() for p in pts], [0, 0, 1])
    bad = (T0 + H, struct.pack(">H", (10 << 4) | 7) + struct.pack(">H", (20 << 4) | 7), b"\x01\x02\x00")   # 8-byte values claimed
    d = synth.from_series([[bad]], [0])
    eng.load(a)
    inside, outside = dsq(T0, T0 + 3 * H, "sum", "sum", 60000), dsq(T0, T0 + H, "sum", "sum", 60000)
    before = eng.run(outside)
    eng.upsert(d, [1], [0])
    with pytest.raises(EngineError) as e:
        eng.run(inside)
    assert e.value.java == "IllegalDataException"
    identical(before, eng.run(outside), "outside the malformed row's range")
    eng.load(merge_batches(a, d, [1], [0]))
    with pytest.raises(EngineError) as f:
        eng.run(inside)
    assert (f.value.code, str(f.value)) == (e.value.code, str(e.value))


# ---- 9. load_cells: a row whose compaction fails ------------------------------------------------
@gpu
def test_load_cells_compaction_error(eng):
    from opentsdb_amd.engine import EngineError
    rng = np.random.default_rng(11)
    good = [int_points(rng, T0 + np.arange(0, 3 * H, 60), 0, 1000) for _ in range(4)]
    q1 = struct.pack(">H", (10 << 4) | 0)
    q2 = struct.pack(">H", (20 << 4) | 0)
    cells = lambda rows: [(b, [(q, v, None)]) for b, q, v in rows]   # noqa: E731
    # series 1's MIDDLE row fails to compact: a second twice, with another value
    bad_row = (T0 + H, [(q1, b"\x01", None), (q1 + q2, b"\x02\x03\x00", None)])
    series = [cells(good[0].rows()), cells(good[1].rows(None, T0 + H)) + [bad_row] + cells(good[1].rows(T0 + 2 * H, None)),
              cells(good[2].rows())]
    q = dsq(T0, T0 + 3 * H, "sum", "sum", 600000)

    def load():
        eng.load_cells(abi.HostCellBatch.from_rows(series, [0, 0, 1]))
        with pytest.raises(EngineError) as e0:
            eng.run(q)
        assert e0.value.java == "IllegalDataException"
        return e0

    # an upsert elsewhere keeps the error, under the renumbered index: a new series in front
    e0 = load()
    d = synth.from_series([good[3].rows(), good[0].rows(T0 + H, T0 + 2 * H)], [1, 0])
    eng.upsert(d, [0, 1], [1, 0])
    with pytest.raises(EngineError) as e1:
        eng.run(q)
    assert (e1.value.code, str(e1.value)) == (e0.value.code, str(e0.value))
    eng.regroup([1, 0, EXCL, 1])          # the bad series is index 2 now
    want = O.run_query(synth.from_series([good[3].rows(), good[0].rows(), good[2].rows()], [1, 0, 1]), q)
    assert_groups_match(eng.run(q), want, "sum", tol=0.0, ctx="bad series excluded by its new index")
    eng.regroup([1, EXCL, 0, 1])
    with pytest.raises(EngineError):
        eng.run(q)
    # an upsert that brings that (series, base) in the middle clears the error
    load()
    eng.upsert(synth.from_series([good[1].rows(T0 + H, T0 + 2 * H)], [0]), [1], [0])
    want = O.run_query(synth.from_series([good[0].rows(), good[1].rows(), good[2].rows()], [0, 0, 1]), q)
    assert_groups_match(eng.run(q), want, "sum", tol=0.0, ctx="bad row replaced")


# ---- 10. rollup / pre-aggregate cells -----------------------------------------------------------
@gpu
def test_rollup_and_preagg_cells(eng):
    from opentsdb_amd import engine
    rng = np.random.default_rng(31)
    pts = [quarter_points(rng, T0 + np.arange(0, 3 * H, 300)) for _ in range(6)]
    a, d, idx, new, full = upsert_case(pts, [0, 0, 1, 1, 2, NONE], [[(T0 + H, T0 + 2 * H)]] * 6, [[T0 + H]] * 6,
                                       resident=[True, True, False, True, True, True])
    iv = engine.rollup_interval("10m", "1d")
    end = T0 + 3 * H
    eng.load(a)
    old = eng.rollup(iv, T0, end, FUNCS)
    assert len(old) and eng.preagg_run(iv, T0, end, "sum", FUNCS)[0]
    eng.upsert(d, idx, new)
    ser = np.full(len(old), -7, np.int32)
    voff = np.full(len(old) + 1, 2 ** 63, np.uint64)
    assert engine.lib().tsdbhip_rollup_download(eng.ctx, ser.ctypes.data, None, None, voff.ctypes.data, None) == 0
    assert voff[0] == 0 and (ser == -7).all()
    assert resident_cells(eng) == 0
    cells = eng.rollup(iv, T0, end, FUNCS)
    pre = eng.preagg(iv, T0, end, "sum", FUNCS)
    assert len(cells) > len(old) and len(pre)
    eng.load(full)
    fresh = eng.rollup(iv, T0, end, FUNCS)
    for name in ("series", "base_time", "qualifier", "val_off", "value"):
        np.testing.assert_array_equal(getattr(cells, name), getattr(fresh, name), err_msg=name)
    fpre = eng.preagg(iv, T0, end, "sum", FUNCS)
    for name in ("func_index", "group", "base_time", "qual_off", "qualifier", "val_off", "value"):
        np.testing.assert_array_equal(getattr(pre, name), getattr(fpre, name), err_msg=name)


# ---- 11. refusals and atomicity -----------------------------------------------------------------
def upsert_code(e, d, idx, new, info=True):
    from opentsdb_amd import engine
    idx = np.ascontiguousarray(idx, np.int64)
    new = np.ascontiguousarray(new, np.uint8)
    inf = abi.UpsertInfo()
    return engine.lib().tsdbhip_upsert(e.ctx, C.byref(d.c) if d is not None else None,
                                       idx.ctypes.data if len(idx) else None,
                                       new.ctypes.data if len(new) else None, C.byref(inf) if info else None)


@gpu
def test_refused_calls_leave_the_batch(eng):
    from opentsdb_amd import engine
    from tests.test_gpu_append import append_code
    pts, gids = small_store()
    a, d, idx, new, full = split(pts, gids, T0 + 2 * H + 900, resident=[True, True, False, True, True])
    qs = [dsq(T0, T0 + 3 * H, "sum", "sum", 600000), dsq(T0, T0 + 3 * H, "none", "sum", 600000)]
    eng.load(a)
    before = [eng.run(q) for q in qs]
    sz = sizes(eng)
    IA, NI = abi.TSDB_E_ILLEGAL_ARGUMENT, abi.TSDB_E_NOT_IMPLEMENTED

    def unchanged(ctx):
        assert sizes(eng) == sz, ctx
        for i, (q, b) in enumerate(zip(qs, before)):
            identical(b, eng.run(q), f"after {ctx} q{i}")

    assert engine.lib().tsdbhip_upsert(eng.ctx, None, None, None, None) == IA
    assert engine.lib().tsdbhip_upsert(eng.ctx, C.byref(d.c), None, None, None) == IA
    unchanged("null pointers")
    bad = idx.copy(); bad[0] = 5                       # N' = 5: outside [0, N')
    assert upsert_code(eng, d, bad, new) == IA
    bad = idx.copy(); bad[0] = -1
    assert upsert_code(eng, d, bad, new) == IA
    bad = idx.copy(); bad[1] = bad[0]                  # repeated
    assert upsert_code(eng, d, bad, new) == IA
    unchanged("indices")
    assert upsert_code(eng, with_ids(d, [0, 0, -3, 0, 0]), idx, new) == IA   # a new series' id below -2
    broken = abi.HostBatch(d.series_row_ptr.copy(), d.row_base_time, d.row_qual_off, d.row_val_off, d.qual, d.val, d.group_id)
    broken.series_row_ptr[-1] -= 1                      # does not cover the rows
    assert upsert_code(eng, broken, idx, new) == IA
    broken = abi.HostBatch(d.series_row_ptr.copy(), d.row_base_time, d.row_qual_off, d.row_val_off, d.qual, d.val, d.group_id)
    broken.series_row_ptr[1], broken.series_row_ptr[2] = broken.series_row_ptr[2], broken.series_row_ptr[1] - 1
    assert upsert_code(eng, broken, idx, new) == IA     # not monotonic
    unchanged("delta invariants")
    # the two deltas tsdbhip_append refuses: it still does, and names the way out
    back = synth.from_series([pts[0].rows(T0 + H, T0 + 2 * H)], [0])
    assert append_code(eng, back, [0], [0]) == NI
    msg = engine.lib().tsdbhip_last_error().decode()
    assert "reload" in msg and "tsdbhip_upsert" in msg
    two = synth.from_series([pts[1].rows(T0 + H, None)], [0])          # replaces the middle row as well
    assert append_code(eng, two, [1], [0]) == NI
    unchanged("back-fill through append")
    assert upsert_code(eng, synth.from_series([], []), [], []) == 0    # an empty delta is a no-op
    unchanged("empty delta")
    # upsert takes both: an identical middle row rewritten; a middle and the last row
    assert upsert_code(eng, back, [0], [0]) == 0
    assert upsert_code(eng, two, [1], [0], info=False) == 0
    cur = merge_batches(merge_batches(a, back, [0], [0]), two, [1], [0])
    assert cur.n_rows == a.n_rows
    rb, _ = restricted(cur, cur.group_id)
    for q in qs:
        assert_groups_match(eng.run(q), want_of(rb, q), agg_name(q), tol=0.0, ctx="after back and two")
    assert upsert_code(eng, d, idx, new) == 0
    assert_groups_match(eng.run(qs[0]), O.run_query(full, qs[0]), "sum", tol=0.0, ctx="after the refusals")


@gpu
def test_not_implemented_contexts(eng):
    from opentsdb_amd import engine
    from opentsdb_amd.rollup_read import make_rollup_batch
    pts, gids = small_store()
    a, d, idx, new, full = split(pts, gids, T0 + 2 * H + 900)
    NI = abi.TSDB_E_NOT_IMPLEMENTED
    iv = engine.rollup_interval("10m", "1d")
    cell = (struct.pack(">H", (0 << 4) | 0x7), struct.pack(">q", 5))
    eng.load_rollup(make_rollup_batch([(None, [(T0, [cell], [])])], [0], iv, False))
    assert upsert_code(eng, d, idx, new) == NI
    eng.load_shard(a, engine.SHARD_SPANS, 0, a.n_series)
    q = dsq(T0, T0 + 3 * H, "sum", "sum", 600000)
    before = eng.run(q)
    assert upsert_code(eng, d, idx, new) == NI
    identical(before, eng.run(q), "shard batch untouched")
    md = engine.Engine(devices=[0, 0])
    try:
        md.load(a)
        before = md.run(q)
        assert upsert_code(md, d, idx, new) == NI
        identical(before, md.run(q), "multi-device context untouched")
    finally:
        md.close()
    # an upsert onto an empty load is legal
    eng.load(synth.from_series([], []))
    info = eng.upsert(full, np.arange(full.n_series), np.ones(full.n_series))
    assert info.series_added == full.n_series and info.rows_added == full.n_rows
    assert_groups_match(eng.run(q), O.run_query(full, q), "sum", tol=0.0, ctx="onto an empty load")


# ---- 12. real tiles -----------------------------------------------------------------------------
@gpu
def test_real_tiles(eng):
    """131 072 series x three hour rows of 12 small integers (T = 64, the grid-stride loop).  One
    delta replaces the middle row of every third series, inserts a row before the first of every
    fifth and adds 1000 new series spread over the batch.  Every series has a point in every
    five-minute bucket between its first and last point."""
    n, k = 131072, 1000
    eng.synth(n, T0, 36, 300000, 1, 4, 1000)
    a = eng.download()
    assert a.n_series == n and a.n_rows == 3 * n
    n2 = n + k
    is_new = np.zeros(n2, bool)
    is_new[np.arange(k) * (n2 // k) + 7] = True
    old_of = np.cumsum(~is_new) - 1
    front = ~is_new & (old_of % 5 == 0)                   # a row at T0 - H
    mid = np.where(is_new, True, old_of % 3 == 0)         # a row at T0 + H: the replacement, or a new series' only row
    idx = np.flatnonzero(front | mid)
    pair = np.stack([front[idx], mid[idx]], axis=1)
    bases = np.tile(np.array([T0 - H, T0 + H], np.uint32), len(idx))[pair.ravel()]
    nr = len(bases)
    rng = np.random.default_rng(77)
    offs = np.tile(np.arange(12, dtype=np.uint16) * 300, (nr, 1))
    qual = (offs << 4).astype(">u2").view(np.uint8).ravel()
    val = np.zeros((nr, 13), np.uint8)
    val[:, :12] = rng.integers(0, 128, (nr, 12))
    srp = np.zeros(len(idx) + 1, np.int64)
    srp[1:] = np.cumsum(pair.sum(axis=1))
    d = abi.HostBatch(srp, bases, np.arange(nr + 1, dtype=np.uint64) * 24, np.arange(nr + 1, dtype=np.uint64) * 13,
                      qual, val.ravel(), (idx % 4).astype(np.int32))
    queries = [dsq(T0 - H, T0 + 3 * H, "sum", "sum", 300000), dsq(T0 - H, T0 + 3 * H, "max", "max", 300000)]
    for q in queries:
        eng.run(q)
    info = eng.upsert(d, idx, is_new[idx])
    assert (info.series_added, info.rows_replaced, info.rows_reindexed) == (k, (n + 2) // 3, 0)
    assert info.rows_added == nr - info.rows_replaced
    m = merge_batches(a, d, idx, is_new[idx])
    assert sizes(eng) == (n2, m.n_rows, int(m.row_qual_off[-1]), int(m.row_val_off[-1]))
    for i, q in enumerate(queries):
        got = eng.run(q)
        assert len(got) == 4
        assert_groups_match(got, O.run_query(m, q, threads=8), agg_name(q), tol=0.0, ctx=f"real tiles q{i}")


# ---- 13. ResidentSpans end to end ---------------------------------------------------------------
@gpu
def test_resident_spans_refresh_equals_tsdb_query(eng):
    from opentsdb_amd.query import ResidentSpans
    from tests.test_append_cpu import growing_store
    from tests.test_regroup_cpu import METRIC, QUERIES, START, query
    from tests.test_upsert_cpu import late_writes
    end = START + 3 * 3600
    # TsdbQuery.run() over the store as it will stand (it loads batches of its own: asked first)
    after, _ = growing_store(end)
    late_writes(after)
    want = {}
    for i, tags in enumerate(QUERIES):
        q = query(after, tags, start=START, end=end - 1)
        q.runner = eng.run_batch
        want[i] = q.run()
    st, _ = growing_store(end)
    rs = ResidentSpans(st, METRIC, START, end, engine=eng)
    rs.run(query(st, {"host": "*"}, start=START, end=end - 1))     # the old state
    late_writes(st)                                               # an old hour rewritten, late points, a back-filled series
    info = rs.refresh(START + 3600, START + 7200)
    assert info.series_added == 1 and info.rows_added == 1 and info.rows_replaced == 10
    for i, tags in enumerate(QUERIES):
        exp = want[i]
        got = rs.run(query(st, tags, start=START, end=end - 1))
        assert len(got) == len(exp), tags
        by = {d.group_key: d for d in got}
        for d in exp:
            g = by[d.group_key]
            for name in ("ts", "bits", "is_int"):
                np.testing.assert_array_equal(getattr(g, name), getattr(d, name), err_msg=f"{tags} {name}")
