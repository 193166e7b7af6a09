"""GPU parity of tsdbhip_append (k_append.hip): newly scanned rows appended to the resident batch
without a reload.

The expectation never comes from the engine: after load(A) + append(D) the context must answer
as a fresh load of merge_batches(A, D) would (tests/append_util.py, checked against stores built
from full point lists in tests/test_append_cpu.py).  Every case first queries the OLD state over
the old range (stale caches would show), appends, compares every query with the oracle over the
merged batch restricted to its visible series bit for bit (tol = 0.0), and then compares
results, debug_rows() and download() array for array with the same engine after a fresh load of
that batch.

Inputs are order-free -- integers, or multiples of 0.25 below 2^20 (the stores of
tests/test_gpu_regroup.py) -- so the default unordered path must equal the oracle to the bit;
`dev` and full-mantissa floats run under TSDB_QF_ORDERED."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import pytest

from opentsdb_amd import abi, synth
from oracle import oracle as O
from tests.append_util import (Points, batches_equal, int_points, merge_batches, quarter_points, split, with_ids)
from tests.test_gpu_parity import assert_groups_match
from tests.test_gpu_preagg import FUNCS, resident_cells
from tests.test_gpu_regroup import agg_name, dsq, identical, resident_order, restricted, want_of

gpu = pytest.mark.gpu

T0 = 1356998400
H = 3600
EXCL = abi.GROUP_EXCLUDED
NONE = abi.GROUP_NONE


@pytest.fixture(scope="module")
def eng():
    from opentsdb_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def sizes(e):
    from opentsdb_amd import engine
    ns, nr, qb, vb = C.c_int64(), C.c_int64(), C.c_uint64(), C.c_uint64()
    assert engine.lib().tsdbhip_batch_sizes(e.ctx, C.byref(ns), C.byref(nr), C.byref(qb), C.byref(vb)) == 0
    return ns.value, nr.value, qb.value, vb.value


def state(e, queries):
    return [e.run(q) for q in queries], e.debug_rows(), e.download(), sizes(e), e.resident_groups()


def same_state(got, fresh, queries, ctx):
    for i, (g, f) in enumerate(zip(got[0], fresh[0])):
        identical(g, f, f"{ctx} q{i} vs fresh load")
    for name, x, y in zip(("ndp", "flags", "lsb", "absmax"), got[1], fresh[1]):
        np.testing.assert_array_equal(x, y, err_msg=f"{ctx} debug_rows {name}")
    batches_equal(got[2], fresh[2])
    assert got[3] == fresh[3], ctx
    np.testing.assert_array_equal(got[4], fresh[4])


def check_append(eng, a, d, idx, new, queries, ctx, loaded=False, old_queries=None, full=None):
    """One case.  `a` carries the PRESENT ids of the resident series (GROUP_EXCLUDED included,
    when the caller has regrouped).  Returns (info, results, merged batch)."""
    if not loaded:
        eng.load(a)
    for q in (queries if old_queries is None else old_queries):
        eng.run(q)                                   # the old state
    info = eng.append(d, idx, new)
    m = merge_batches(a, d, idx, new)
    if full is not None:
        batches_equal(m, full)
    rb, kept = restricted(m, m.group_id)
    assert eng.n_series() == len(kept), ctx
    got = state(eng, queries)
    for i, (q, g) in enumerate(zip(queries, got[0])):
        assert_groups_match(g, want_of(rb, q), agg_name(q), tol=0.0, ctx=f"{ctx} q{i} vs oracle")
    np.testing.assert_array_equal(got[4], resident_order(rb.group_id))
    assert got[3] == (rb.n_series, rb.n_rows, int(rb.row_qual_off[-1]), int(rb.row_val_off[-1])), ctx
    assert info.series_added == int(np.count_nonzero(new))
    eng.load(rb)
    same_state(got, state(eng, queries), queries, ctx)
    return info, got[0], m


# ---- row-class changes at tile size 1 -----------------------------------------------------------
def mixed_points(rng, ts_s, s):
    """Integer, float32 and float64 values in one row; millisecond qualifiers on every other series."""
    ts = np.asarray(ts_s, np.int64) * 1000 + (250 if s % 2 else 0)
    n = len(ts)
    kind = rng.integers(0, 3, n)
    fv = rng.integers(1, 1 << 22, n).astype(np.float64) * 0.25
    fv[kind == 2] += float(2 ** 25)
    return Points(ts, rng.integers(-5000, 5000, n), fv, kind, np.full(n, bool(s % 2)))


def class_case(name):
    """(points, cut, end): the store's full point lists, the clock at the load, the new scan end."""
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    if name == "short_f32":      # one 360-point row a series gains a second hour row: k_short -> k_rows
        return [quarter_points(rng, T0 + np.arange(0, 2 * H, 10)) for _ in range(12)], T0 + H, T0 + 2 * H
    if name == "short_int":
        return [int_points(rng, T0 + np.arange(0, 2 * H, 10), -100, 30000) for _ in range(12)], T0 + H, T0 + 2 * H
    if name == "rows":           # gains a row, and its last row is replaced by a longer one
        return [quarter_points(rng, T0 + np.arange(0, 4 * H, 30)) for _ in range(10)], T0 + 2 * H + 1800, T0 + 4 * H
    if name == "walker":         # a 3000-point row replaced by the 3600-point one
        return [quarter_points(rng, T0 + np.arange(0, H, 1)) for _ in range(9)], T0 + 3000, T0 + H
    if name == "mixed":          # ms, float64 and vle rows appended
        return [mixed_points(rng, T0 + np.arange(0, 3 * H, 20), s) for s in range(12)], T0 + H + 1200, T0 + 3 * H
    raise KeyError(name)


CLASSES = ["short_f32", "short_int", "rows", "walker", "mixed"]


@gpu
@pytest.mark.parametrize("name", CLASSES)
def test_row_classes(eng, name):
    pts, cut, end = class_case(name)
    a, d, idx, new, full = split(pts, [i % 3 for i in range(len(pts))], cut)
    queries = [dsq(T0, end, "sum", "sum", 60000), dsq(T0, end, "max", "max", 60000)]
    if name == "short_int":
        queries += [abi.new_query(T0, end - 1, "sum"), dsq(T0, end, "p99", "avg", 60000)]
    old = [dsq(T0, cut, "sum", "sum", 60000), dsq(T0, cut, "max", "max", 60000)]
    info, got, _ = check_append(eng, a, d, idx, new, queries, name, old_queries=old, full=full)
    assert len(got[0]) == 3
    assert info.rows_added + info.rows_replaced == d.n_rows
    assert info.rows_replaced == (0 if name.startswith("short") else len(pts))


@gpu
def test_ordered_full_mantissa(eng):
    """Full 53-bit mantissa float64 and `dev` under TSDB_QF_ORDERED."""
    rng = np.random.default_rng(4)
    pts = [Points((T0 + np.arange(720) * 10) * 1000, fvals=45.0 + 10.0 * rng.random(720), kind=np.full(720, 2))
           for _ in range(12)]
    a, d, idx, new, fb = split(pts, [i % 2 for i in range(12)], T0 + H + 900)
    queries = [dsq(T0, T0 + 2 * H, "sum", "sum", 60000, flags=abi.QF_ORDERED),
               dsq(T0, T0 + 2 * H, "dev", "avg", 600000, flags=abi.QF_ORDERED)]
    check_append(eng, a, d, idx, new, queries, "ordered f64", full=fb)


# ---- val2 -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("opts", [{}, {"INDEX_FUSED": 0}, {"INDEX_GENERIC": 1}], ids=["default", "unfused", "generic"])
@pytest.mark.parametrize("kind", ["float_then_int", "int_then_int"])
def test_val2(eng, kind, opts):
    """The int16 copy of 1-2-byte integer values lives at qualifier offsets: it appears with the
    first delta row that needs it (a float-only load has none), and it grows with the qualifier
    blob while old rows still read it."""
    from opentsdb_amd import engine
    rng = np.random.default_rng(3)
    n = 10
    ts = T0 + np.arange(0, 2 * H, 10)
    if kind == "float_then_int":
        pts = [quarter_points(rng, ts[ts < T0 + H]) if s % 2 else int_points(rng, ts, -100, 30000) for s in range(n)]
        resident = [bool(s % 2) for s in range(n)]    # the integer series are new: the load is float-only
    else:
        pts = [int_points(rng, ts, -100, 30000) for _ in range(n)]
        resident = [True] * n
    a, d, idx, new, full = split(pts, [s % 3 for s in range(n)], T0 + H + 600, resident=resident)
    queries = [dsq(T0, T0 + 2 * H, "sum", "sum", 60000), dsq(T0, T0 + 2 * H, "max", "max", 60000),
               abi.new_query(T0, T0 + 2 * H - 1, "sum")]
    with engine.options(**opts):
        check_append(eng, a, d, idx, new, queries, f"{kind} {opts}", full=full)


# ---- replace --------------------------------------------------------------------------------------
@gpu
def test_replace_only_row_shorter_row_and_three_times(eng):
    rng = np.random.default_rng(5)
    n = 7
    pts = [int_points(rng, T0 + np.arange(0, H, 10), -100, 30000) for _ in range(n)]
    gids = [s % 2 for s in range(n)]
    queries = [dsq(T0, T0 + H, "sum", "sum", 60000), dsq(T0, T0 + H, "max", "max", 60000)]
    # the only row of every series replaced (ROW_SFIRST comes from the gather)
    a, d, idx, new, full = split(pts, gids, T0 + 1800)
    info, _, _ = check_append(eng, a, d, idx, new, queries, "only row", full=full)
    assert (info.rows_added, info.rows_replaced) == (0, n)
    # ... by a shorter one
    short = synth.from_series([p.rows(T0, T0 + 600) for p in pts], gids)
    info, _, _ = check_append(eng, a, short, np.arange(n), np.zeros(n), queries, "shorter row")
    assert (info.rows_added, info.rows_replaced) == (0, n)
    # the same row three times: the dead bytes are the replaced rows' aligned lengths
    al = lambda x: (int(x) + 15) & ~15   # noqa: E731
    four = np.arange(4)
    cur = a
    eng.load(a)
    dead_q = dead_v = 0
    for hi in (T0 + 2400, T0 + 3000, T0 + H):
        dd = synth.from_series([p.rows(T0, hi) for p in pts[:4]], gids[:4])
        dead_q += sum(al(x) for x in np.diff(cur.row_qual_off)[:4])      # (one row a series: rows 0..3)
        dead_v += sum(al(x) for x in np.diff(cur.row_val_off)[:4])
        info = eng.append(dd, four, np.zeros(4))
        cur = merge_batches(cur, dd, four, np.zeros(4))
        assert (info.rows_added, info.rows_replaced) == (0, 4)
        assert (info.qual_dead, info.val_dead) == (dead_q, dead_v), hi
        assert sizes(eng) == (cur.n_series, cur.n_rows, int(cur.row_qual_off[-1]), int(cur.row_val_off[-1]))
    got = state(eng, queries)
    for i, (q, g) in enumerate(zip(queries, got[0])):
        assert_groups_match(g, O.run_query(cur, q), agg_name(q), tol=0.0, ctx=f"three replacements q{i}")
    eng.load(cur)
    same_state(got, state(eng, queries), queries, "three replacements")


# ---- new series -------------------------------------------------------------------------------------
@gpu
def test_new_series_positions_and_ids(eng):
    """New series first, in the middle of a group and last in batch order; with an id beyond
    n_groups, GROUP_NONE and GROUP_EXCLUDED; first / last / diff show the order inside the group;
    a series resident with zero rows receives its first row."""
    rng = np.random.default_rng(8)
    n = 12
    ts = T0 + np.arange(0, 2 * H, 60)
    pts = [int_points(rng, ts, -1000, 1000) for _ in range(n)]
    pts[5] = int_points(rng, ts[ts >= T0 + H + 1800], -1000, 1000)        # resident, no row before the cut
    #        0  1  2  3  4  5  6  7     8  9  10    11
    gids = [0, 1, 0, 1, 0, 1, 0, NONE, 0, 4, EXCL, 1]
    resident = [i not in (0, 4, 7, 9, 10, 11) for i in range(n)]          # resident: groups 0 and 1 only
    a, d, idx, new, full = split(pts, gids, T0 + H + 600, resident=resident)
    assert a.n_series == 6 and int(a.series_row_ptr[3] - a.series_row_ptr[2]) == 2 and set(a.group_id.tolist()) == {0, 1}
    assert int(a.series_row_ptr[4]) == int(a.series_row_ptr[3])            # series 5 of the store: zero rows in A
    end = T0 + 2 * H
    queries = [dsq(T0, end, a_, "sum", 600000) for a_ in ("first", "last", "diff", "sum", "none")]
    queries.append(abi.new_query(T0, end - 1, "mult"))
    info, got, m = check_append(eng, a, d, idx, new, queries, "new series", full=full)
    assert info.series_added == 6 and [g for g, *_ in got[3]] == [0, 1, 4]
    assert len(got[4]) == 11                                              # NONE emits every visible span


# ---- with regroup ---------------------------------------------------------------------------------
@gpu
def test_with_regroup(eng):
    rng = np.random.default_rng(13)
    n = 9
    pts = [quarter_points(rng, T0 + np.arange(0, 3 * H, 30)) for _ in range(n)]
    a, d, idx, new, full = split(pts, [0] * n, T0 + 2 * H + 600, resident=[True] * 4 + [False] + [True] * 4)
    assert a.n_series == 8 and int(new.sum()) == 1 and idx[4] == 4
    d = with_ids(d, np.where(new != 0, 2, 0))
    ids = np.array([1, EXCL, 0, 0, EXCL, 1, NONE, 0], np.int32)
    end = T0 + 3 * H
    queries = [dsq(T0, end, "sum", "sum", 60000), dsq(T0, end, "none", "sum", 600000)]
    eng.load(a)
    eng.regroup(ids)
    _, got, m = check_append(eng, with_ids(a, ids), d, idx, new, queries, "after regroup", loaded=True)
    assert [g for g, *_ in got[0]] == [0, 1, 2]
    # a later regroup, ids in the NEW index space, readmits the excluded series with their appended rows
    eng.load(a)
    eng.regroup(ids)
    eng.append(d, idx, new)
    ids2 = np.array([0, 1, EXCL, 0, 1, 1, 0, 0, NONE], np.int32)
    eng.regroup(ids2)
    got = state(eng, queries)
    rb, kept = restricted(full, ids2)
    for i, (q, g) in enumerate(zip(queries, got[0])):
        assert_groups_match(g, want_of(rb, q), agg_name(q), tol=0.0, ctx=f"readmitted q{i}")
    eng.load(rb)
    same_state(got, state(eng, queries), queries, "readmitted")


# ---- growth ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("reserve", [0, None], ids=["exact", "default"])
def test_growth(eng, reserve):
    from opentsdb_amd import engine
    rng = np.random.default_rng(21)
    n = 8
    # five hours resident, three more appended: 1.5 x the first need holds the other two
    pts = [quarter_points(rng, T0 + np.arange(0, 9 * H, 30)) for _ in range(n)]
    gids = [s % 2 for s in range(n)]
    end = T0 + 8 * H
    queries = [dsq(T0, end, "sum", "sum", 60000), dsq(T0, end, "max", "max", 60000)]
    cur = synth.from_series([p.rows(None, T0 + 5 * H + 600) for p in pts], gids)
    with engine.options(APPEND_RESERVE=reserve):
        eng.load(cur)
        grew, caps = [], []
        for k in (5, 6, 7):   # each rescan: the live hour's row replaced, the next hour begun
            dd = synth.from_series([p.rows(T0 + k * H, T0 + (k + 1) * H + 600) for p in pts], gids)
            for q in queries:
                eng.run(q)
            info = eng.append(dd, np.arange(n), np.zeros(n))
            cur = merge_batches(cur, dd, np.arange(n), np.zeros(n))
            grew.append(info.grew)
            caps.append((info.qual_capacity, info.val_capacity))
            assert (info.rows_added, info.rows_replaced) == (n, n)
        got = state(eng, queries)
    assert grew == ([1, 1, 1] if reserve == 0 else [1, 0, 0]), (grew, caps)
    if reserve is None:
        assert caps[0] == caps[1] == caps[2]
    batches_equal(cur, synth.from_series([p.rows(None, end + 600) for p in pts], gids))
    for i, (q, g) in enumerate(zip(queries, got[0])):
        assert_groups_match(g, O.run_query(cur, q), agg_name(q), tol=0.0, ctx=f"growth {reserve} q{i}")
    eng.load(cur)
    same_state(got, state(eng, queries), queries, f"growth {reserve}")


# ---- k_recede --------------------------------------------------------------------------------------
def sec_row(base, offs, vals):
    """A compacted row of 2-byte second qualifiers (offsets up to 4095 s) and 1-byte integers."""
    q = b"".join(struct.pack(">H", (o << 4) | 0) for o in offs)
    v = bytes(x & 0xFF for x in vals) + (b"\x00" if len(offs) > 1 else b"")
    return (base, q, v)


@gpu
def test_recede_across_the_appended_row(eng):
    """The last resident row ends with an offset past the hour (3700 s), the appended next-hour
    row starts before it (3610 s): the delta row carries ROW_UNSORTED as the fresh load's does."""
    rows_a = [[sec_row(T0, [0, 600, 1200, 3700], [1, 2, 3, 4])], [sec_row(T0, [0, 900], [5, 6])],
              [sec_row(T0, [30, 3650], [7, 8]), ]]
    a = synth.from_series(rows_a, [0, 0, 1])
    rows_d = [[sec_row(T0 + H, [10, 50, 700], [9, 10, 11])], [sec_row(T0 + H, [5, 60], [12, 13])],
              [sec_row(T0 + H, [100, 40, 900], [14, 15, 16])]]      # the last: a cell unsorted in itself
    d = synth.from_series(rows_d, [0, 0, 1])
    queries = [dsq(T0, T0 + 2 * H, "sum", "sum", 60000), abi.new_query(T0, T0 + 2 * H - 1, "sum")]
    eng.load(a)
    check_append(eng, a, d, np.arange(3), np.zeros(3), queries, "recede", loaded=True)
    eng.load(a)
    eng.append(d, np.arange(3), np.zeros(3))
    flags = eng.debug_rows()[1]
    UNSORTED = 0x100000
    # resident order: group 0 (series 0, 1), group 1 (series 2); two rows each
    assert [bool(f & UNSORTED) for f in flags] == [False, True, False, False, False, True]


@gpu
def test_malformed_delta_cell_is_reported_lazily(eng):
    from opentsdb_amd.engine import EngineError
    rng = np.random.default_rng(2)
    pts = [int_points(rng, T0 + np.arange(0, H, 60), 0, 100) for _ in range(3)]
    a = synth.from_series([p.rows() for p in pts], [0, 0, 1])
    bad = (T0 + H, struct.pack(">H", (10 << 4) | 7) + struct.pack(">H", (20 << 4) | 7), b"\x01\x02\x00")   # 8-byte values claimed
    d = synth.from_series([[bad]], [0])
    eng.load(a)
    inside, outside = dsq(T0, T0 + 2 * H, "sum", "sum", 60000), dsq(T0, T0 + H, "sum", "sum", 60000)
    before = eng.run(outside)
    eng.append(d, [1], [0])
    with pytest.raises(EngineError) as e:
        eng.run(inside)
    assert e.value.java == "IllegalDataException"
    identical(before, eng.run(outside), "outside the malformed row's range")
    eng.load(merge_batches(a, d, [1], [0]))
    with pytest.raises(EngineError) as f:
        eng.run(inside)
    assert (f.value.code, str(f.value)) == (e.value.code, str(e.value))


# ---- load_cells: a row whose compaction fails ---------------------------------------------------
@gpu
def test_load_cells_compaction_error(eng):
    from opentsdb_amd.engine import EngineError
    rng = np.random.default_rng(11)
    good = [int_points(rng, T0 + np.arange(0, 2 * H, 60), 0, 1000) for _ in range(4)]
    q1 = struct.pack(">H", (10 << 4) | 0)
    q2 = struct.pack(">H", (20 << 4) | 0)
    cells = lambda rows: [(b, [(q, v, None)]) for b, q, v in rows]   # noqa: E731
    # series 1's last row (the second hour) fails to compact: a second twice, with another value
    bad_row = (T0 + H, [(q1, b"\x01", None), (q1 + q2, b"\x02\x03\x00", None)])
    series = [cells(good[0].rows(None, T0 + H)), cells(good[1].rows(None, T0 + H)) + [bad_row],
              cells(good[2].rows())]
    q = dsq(T0, T0 + 2 * H, "sum", "sum", 600000)

    def load():
        eng.load_cells(abi.HostCellBatch.from_rows(series, [0, 0, 1]))
        with pytest.raises(EngineError) as e0:
            eng.run(q)
        assert e0.value.java == "IllegalDataException"
        return e0

    # an append elsewhere keeps the error, under the renumbered index: a new series in front
    e0 = load()
    d = synth.from_series([good[3].rows(), good[0].rows(T0 + H, None)], [1, 0])
    eng.append(d, [0, 1], [1, 0])
    with pytest.raises(EngineError) as e1:
        eng.run(q)
    assert (e1.value.code, str(e1.value)) == (e0.value.code, str(e0.value))
    eng.regroup([1, 0, EXCL, 1])          # the bad series is index 2 now
    want = O.run_query(synth.from_series([good[3].rows(), good[0].rows(), good[2].rows()], [1, 0, 1]), q)
    assert_groups_match(eng.run(q), want, "sum", tol=0.0, ctx="bad series excluded by its new index")
    eng.regroup([1, EXCL, 0, 1])
    with pytest.raises(EngineError):
        eng.run(q)
    # an append that brings that row anew clears the error
    load()
    eng.append(synth.from_series([good[1].rows(T0 + H, None)], [0]), [1], [0])
    want = O.run_query(synth.from_series([good[0].rows(None, T0 + H), good[1].rows(), good[2].rows()], [0, 0, 1]), q)
    assert_groups_match(eng.run(q), want, "sum", tol=0.0, ctx="bad row replaced")


# ---- real tiles ------------------------------------------------------------------------------
@gpu
def test_real_tiles(eng):
    """524 288 series x 12 points (T = 64).  One delta replaces every third series' row with an
    18-point one, adds a next-hour row to every fifth and inserts 1000 new series spread over the
    batch.  (Values are integers below 128.)"""
    n, k = 524288, 1000
    eng.synth(n, T0, 12, 10000, 1, 4, 1000)
    a = eng.download()
    assert a.n_series == n and a.n_rows == n
    n2 = n + k
    is_new = np.zeros(n2, bool)
    is_new[np.arange(k) * (n2 // k) + 7] = True
    old_of = np.cumsum(~is_new) - 1
    has0 = np.where(is_new, True, old_of % 3 == 0)      # a row at T0: the replacement, or a new series' row
    has1 = ~is_new & (old_of % 5 == 0)                   # a next-hour row
    idx = np.flatnonzero(has0 | has1)
    pair = np.stack([has0[idx], has1[idx]], axis=1)
    bases = np.tile(np.array([T0, T0 + H], np.uint32), len(idx))[pair.ravel()]
    nr = len(bases)
    rng = np.random.default_rng(77)
    # a next-hour row starts 64 one-minute buckets after its series' last bucket at T0 (bucket 1 of a
    # 12-point row, bucket 2 of an 18-point one): the LERP fractions of the gap are k / 64 of integer
    # differences, exact in binary, so that the sums stay order-free
    start = np.where(bases == T0, 0, 300 + 60 * np.repeat(has0[idx], pair.sum(axis=1))).astype(np.uint16)
    offs = start[:, None] + np.arange(18, dtype=np.uint16)[None, :] * 10
    qual = (offs << 4).astype(">u2").view(np.uint8).ravel()
    val = np.zeros((nr, 19), np.uint8)
    val[:, :18] = rng.integers(0, 128, (nr, 18))
    srp = np.zeros(len(idx) + 1, np.int64)
    srp[1:] = np.cumsum(pair.sum(axis=1))
    d = abi.HostBatch(srp, bases, np.arange(nr + 1, dtype=np.uint64) * 36, np.arange(nr + 1, dtype=np.uint64) * 19,
                      qual, val.ravel(), (idx % 4).astype(np.int32))
    queries = [dsq(T0, T0 + 2 * H, "sum", "sum", 60000), dsq(T0, T0 + 2 * H, "max", "max", 60000)]
    for q in queries:
        eng.run(q)
    info = eng.append(d, idx, is_new[idx])
    assert (info.series_added, info.rows_replaced) == (k, (n + 2) // 3)
    assert info.rows_added == nr - info.rows_replaced
    m = merge_batches(a, d, idx, is_new[idx])
    assert sizes(eng) == (n2, m.n_rows, int(m.row_qual_off[-1]), int(m.row_val_off[-1]))
    for i, q in enumerate(queries):
        got = eng.run(q)
        assert len(got) == 4
        assert_groups_match(got, O.run_query(m, q, threads=8), agg_name(q), tol=0.0, ctx=f"real tiles q{i}")


# ---- rollup / pre-aggregate cells ---------------------------------------------------------------
@gpu
def test_rollup_and_preagg_cells(eng):
    from opentsdb_amd import engine
    rng = np.random.default_rng(31)
    pts = [quarter_points(rng, T0 + np.arange(0, 3 * H, 300)) for _ in range(6)]
    a, d, idx, new, full = split(pts, [0, 0, 1, 1, 2, NONE], T0 + 2 * H + 900, resident=[True, True, False, True, True, True])
    iv = engine.rollup_interval("10m", "1d")
    end = T0 + 3 * H
    eng.load(a)
    old = eng.rollup(iv, T0, end, FUNCS)
    assert len(old) and eng.preagg_run(iv, T0, end, "sum", FUNCS)[0]
    eng.append(d, idx, new)
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


# ---- refusals and atomicity -----------------------------------------------------------------------
def append_code(e, d, idx, new, info=True):
    from opentsdb_amd import engine
    idx = np.ascontiguousarray(idx, np.int64)
    new = np.ascontiguousarray(new, np.uint8)
    inf = abi.AppendInfo()
    return engine.lib().tsdbhip_append(e.ctx, C.byref(d.c) if d is not None else None,
                                       idx.ctypes.data if len(idx) else None,
                                       new.ctypes.data if len(new) else None, C.byref(inf) if info else None)


def small_store():
    rng = np.random.default_rng(41)
    pts = [int_points(rng, T0 + np.arange(0, 3 * H, 300), 0, 1000) for _ in range(5)]
    return pts, [0, 1, 0, 1, NONE]


@gpu
def test_refused_calls_leave_the_batch(eng):
    from opentsdb_amd import engine
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

    assert engine.lib().tsdbhip_append(eng.ctx, None, None, None, None) == IA
    assert engine.lib().tsdbhip_append(eng.ctx, C.byref(d.c), None, None, None) == IA
    unchanged("null pointers")
    bad = idx.copy(); bad[0] = 5                       # N' = 5: outside [0, N')
    assert append_code(eng, d, bad, new) == IA
    bad = idx.copy(); bad[0] = -1
    assert append_code(eng, d, bad, new) == IA
    bad = idx.copy(); bad[1] = bad[0]                  # repeated
    assert append_code(eng, d, bad, new) == IA
    unchanged("indices")
    assert append_code(eng, with_ids(d, [0, 0, -3, 0, 0]), idx, new) == IA   # a new series' id below -2
    broken = abi.HostBatch(d.series_row_ptr.copy(), d.row_base_time, d.row_qual_off, d.row_val_off, d.qual, d.val, d.group_id)
    broken.series_row_ptr[-1] -= 1                      # does not cover the rows
    assert append_code(eng, broken, idx, new) == IA
    broken = abi.HostBatch(d.series_row_ptr.copy(), d.row_base_time, d.row_qual_off, d.row_val_off, d.qual, d.val, d.group_id)
    broken.series_row_ptr[1], broken.series_row_ptr[2] = broken.series_row_ptr[2], broken.series_row_ptr[1] - 1
    assert append_code(eng, broken, idx, new) == IA     # not monotonic
    unchanged("delta invariants")
    # back-fill: a row before the series' last resident row; replacing a row that is not the last
    back = synth.from_series([pts[0].rows(T0 + H, T0 + 2 * H)], [0])
    assert append_code(eng, back, [0], [0]) == NI
    assert "reload" in engine.lib().tsdbhip_last_error().decode()
    two = synth.from_series([pts[1].rows(T0 + H, None)], [0])          # replaces the middle row as well
    assert append_code(eng, two, [1], [0]) == NI
    unchanged("back-fill")
    # and the accepted call still works afterwards; an empty delta is a no-op
    assert append_code(eng, synth.from_series([], []), [], []) == 0
    unchanged("empty delta")
    assert append_code(eng, d, idx, new, info=False) == 0
    want = O.run_query(full, qs[0])
    assert_groups_match(eng.run(qs[0]), want, "sum", tol=0.0, ctx="after the refusals")


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
    assert append_code(eng, d, idx, new) == NI
    eng.load_shard(a, engine.SHARD_SPANS, 0, a.n_series)
    q = dsq(T0, T0 + 3 * H, "sum", "sum", 600000)
    before = eng.run(q)
    assert append_code(eng, d, idx, new) == NI
    identical(before, eng.run(q), "shard batch untouched")
    md = engine.Engine(devices=[0, 0])
    try:
        md.load(a)
        before = md.run(q)
        assert append_code(md, d, idx, new) == NI
        identical(before, md.run(q), "multi-device context untouched")
    finally:
        md.close()
    # an append onto an empty load is legal
    eng.load(synth.from_series([], []))
    info = eng.append(full, np.arange(full.n_series), np.ones(full.n_series))
    assert info.series_added == full.n_series and info.rows_added == full.n_rows
    assert_groups_match(eng.run(q), O.run_query(full, q), "sum", tol=0.0, ctx="onto an empty load")


# ---- ResidentSpans end to end --------------------------------------------------------------------
@gpu
def test_resident_spans_extend_equals_tsdb_query(eng):
    from opentsdb_amd.query import ResidentSpans
    from tests.test_append_cpu import growing_store
    from tests.test_regroup_cpu import END, METRIC, QUERIES, START, query
    cut = START + 2 * 3600 + 1500
    st, full = growing_store(cut)
    want = {}
    for i, tags in enumerate(QUERIES):
        q = query(full, tags, start=START, end=END + 7200 - 1)
        q.runner = eng.run_batch
        want[i] = q.run()
    rs = ResidentSpans(st, METRIC, START, START + 3 * 3600, engine=eng)   # (the live hour's row is partial)
    rs.run(query(st, {"host": "*"}, start=START, end=START + 3 * 3600 - 1))     # the old state over the old range
    st.rows = full.rows
    info = rs.extend(END + 7200)
    assert info.series_added == 1 and info.rows_replaced == 10   # (the first-hour series has no live row)
    for i, tags in enumerate(QUERIES):
        got = rs.run(query(st, tags, start=START, end=END + 7200 - 1))
        exp = want[i]
        assert len(got) == len(exp), tags
        by = {d.group_key: d for d in got}
        for d in exp:
            g = by[d.group_key]
            for name in ("ts", "bits", "is_int"):
                np.testing.assert_array_equal(getattr(g, name), getattr(d, name), err_msg=f"{tags} {name}")
    assert len(want[1]) == 10   # ten host values now: late01 has joined
