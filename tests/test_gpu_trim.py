"""GPU parity of tsdbhip_trim (k_trim.hip): old rows evicted from the resident batch and the
blobs re-laid without their dead bytes, without a reload.

The expectation never comes from the engine: after load(A) + trim(c) the context must answer as a
fresh load of trim_batch(A, c) would (tests/trim_util.py, checked against stores built from full
point lists in tests/test_trim_cpu.py).  Every case first queries the OLD state (stale caches
would show), trims, compares every query with the oracle over the trimmed batch restricted to
its visible series bit for bit (tol = 0.0), and then compares results, debug_rows(),
debug_regular()'s array, download() and the batch sizes array for array with the same engine
after a fresh load of that batch.  After a pack the blob offsets themselves are checked against
the exclusive scan of the 16-byte-aligned lengths.

Inputs are order-free -- integers, or multiples of 0.25 below 2^20 -- so the default unordered
path must equal the oracle to the bit; `dev` and full-mantissa floats run under TSDB_QF_ORDERED."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import pytest

from opentsdb_amd import abi, synth
from oracle import oracle as O
from tests.append_util import Points, batches_equal, int_points, merge_batches, quarter_points, with_ids
from tests.test_gpu_append import check_append, class_case, same_state, sec_row, sizes, state
from tests.test_gpu_parity import assert_groups_match
from tests.test_gpu_preagg import FUNCS, resident_cells
from tests.test_gpu_regroup import agg_name, dsq, identical, resident_order, restricted, scatter_ids, want_of
from tests.trim_util import aligned_scan, trim_batch

gpu = pytest.mark.gpu

T0 = 1356998400
H = 3600
EXCL = abi.GROUP_EXCLUDED
NONE = abi.GROUP_NONE
NO_PACK = abi.TRIM_NO_PACK
UNSORTED = 0x100000
PACKS = pytest.mark.parametrize("pack", [NO_PACK, 0], ids=["nopack", "pack"])


@pytest.fixture(scope="module")
def eng():
    from opentsdb_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def check_layout(eng, ctx):
    """The packed layout: every loaded row at the exclusive scan of the aligned lengths, in
    descriptor order.  The visible rows' lengths come from download(); rows of excluded series
    follow them, each past the one before."""
    qoff, voff = eng.debug_layout()
    b = eng.download()
    nv = b.n_rows
    np.testing.assert_array_equal(qoff[:nv], aligned_scan(np.diff(b.row_qual_off.astype(np.int64))), err_msg=f"{ctx} qoff")
    np.testing.assert_array_equal(voff[:nv], aligned_scan(np.diff(b.row_val_off.astype(np.int64))), err_msg=f"{ctx} voff")
    assert (qoff % 16 == 0).all() and (voff % 16 == 0).all(), ctx
    assert (np.diff(qoff.astype(np.int64)) >= 0).all() and (np.diff(voff.astype(np.int64)) >= 0).all(), ctx


def check_trim(eng, a, cutoff, pack, queries, ctx, loaded=False, old_queries=None):
    """One case.  `a` carries the PRESENT ids of the resident series (GROUP_EXCLUDED included, when
    the caller has regrouped).  Returns (info, results, trimmed batch)."""
    if not loaded:
        eng.load(a)
    for q in (queries if old_queries is None else old_queries):
        eng.run(q)                                   # the old state
    n_before = eng.n_series()
    info = eng.trim(cutoff, pack)
    t = trim_batch(a, cutoff)
    rb, kept = restricted(t, t.group_id)
    assert eng.n_series() == len(kept) == n_before, ctx
    assert info.rows_evicted == a.n_rows - t.n_rows, ctx
    assert info.series_emptied == int(np.count_nonzero((np.diff(a.series_row_ptr) > 0) & (np.diff(t.series_row_ptr) == 0))), ctx
    got = state(eng, queries)
    reg = eng.debug_regular()[0]
    for i, (q, g) in enumerate(zip(queries, got[0])):
        assert_groups_match(g, want_of(rb, q), agg_name(q), tol=0.0, ctx=f"{ctx} q{i} vs oracle")
    np.testing.assert_array_equal(got[4], resident_order(rb.group_id))
    assert got[3] == (rb.n_series, rb.n_rows, int(rb.row_qual_off[-1]), int(rb.row_val_off[-1])), ctx
    if pack == 0:
        assert info.packed == 1 and info.qual_dead == 0 and info.val_dead == 0, ctx
        check_layout(eng, ctx)
    elif pack == NO_PACK:
        assert info.packed == 0 and info.qual_reclaimed == 0 and info.val_reclaimed == 0, ctx
    eng.load(rb)
    same_state(got, state(eng, queries), queries, ctx)
    np.testing.assert_array_equal(reg, eng.debug_regular()[0], err_msg=f"{ctx} debug_regular")
    return info, got[0], t


# ---- row classes at tile size 1 -------------------------------------------------------------------
def class_store(name):
    """(points, cutoff, end): stores of 2-4 hour rows a series."""
    if name == "walker":         # 3600-point float32 rows: 7200 B of qualifiers, 14401 B of values
        rng = np.random.default_rng(19)
        return [quarter_points(rng, T0 + np.arange(0, 2 * H, 1)) for _ in range(6)], T0 + H, T0 + 2 * H
    pts, _, end = class_case(name)
    return pts, T0 + H, end


@gpu
@PACKS
@pytest.mark.parametrize("name", ["short_f32", "short_int", "rows", "walker", "mixed"])
def test_row_classes(eng, name, pack):
    pts, cutoff, end = class_store(name)
    a = synth.from_series([p.rows() for p in pts], [i % 3 for i in range(len(pts))])
    queries = [dsq(T0, end, "sum", "sum", 60000), dsq(T0, end, "max", "max", 60000), abi.new_query(T0, end - 1, "sum")]
    if name == "short_int":
        queries.append(dsq(T0, end, "p99", "avg", 60000))
    info, got, t = check_trim(eng, a, cutoff, pack, queries, f"{name} {pack}")
    assert len(got[0]) == 3 and info.rows_evicted == len(pts) and info.series_emptied == 0
    if name.startswith("short"):
        assert t.n_rows == len(pts)                  # one row a series: k_rows' class becomes k_short's


@gpu
@PACKS
def test_ordered_full_mantissa(eng, pack):
    """Full 53-bit mantissa float64 and `dev` under TSDB_QF_ORDERED."""
    rng = np.random.default_rng(4)
    pts = [Points((T0 + np.arange(1080) * 10) * 1000, fvals=45.0 + 10.0 * rng.random(1080), kind=np.full(1080, 2))
           for _ in range(12)]
    a = synth.from_series([p.rows() for p in pts], [i % 2 for i in range(12)])
    queries = [dsq(T0, T0 + 3 * H, "sum", "sum", 60000, flags=abi.QF_ORDERED),
               dsq(T0, T0 + 3 * H, "dev", "avg", 600000, flags=abi.QF_ORDERED)]
    check_trim(eng, a, T0 + H, pack, queries, f"ordered f64 {pack}")


# ---- pack geometry --------------------------------------------------------------------------------
def one_point_rows(rng, hours):
    """`hours` consecutive hourly rows of one 1-byte integer each (one 16-byte word a row)."""
    return [sec_row(T0 + k * H, [int(rng.integers(0, 3000))], [int(rng.integers(1, 100))]) for k in range(hours)]


@gpu
@pytest.mark.parametrize("tail", ["exact", "past"])
def test_pack_geometry(eng, tail):
    """The smallest shapes at which the copy kernel can go wrong, in one batch: one-word rows, rows
    of exactly 16 qualifier bytes, 1-KB and 7.2-KB rows, fifty one-word rows a series (one wave
    span of 4 KB holds more rows than lanes), a last row that ends on a 16-byte boundary or one
    byte past it -- scattered by a regroup to a hash order, with dead bytes left by an append."""
    rng = np.random.default_rng(29)
    series = []
    series += [one_point_rows(rng, 2) for _ in range(3)]
    series += [int_points(rng, T0 + np.arange(8) * 60, -100, 100).rows() for _ in range(2)]             # qlen 16
    series += [quarter_points(rng, T0 + np.arange(512) * 7).rows() for _ in range(2)]                   # 1024 B
    series += [quarter_points(rng, T0 + np.arange(0, 2 * H, 1)).rows() for _ in range(2)]               # 3600 dp
    series += [int_points(rng, T0 + np.arange(0, H, 10), -100, 30000).rows() for _ in range(2)]         # vle: val2
    series += [one_point_rows(rng, 50) for _ in range(6)]
    if tail == "exact":          # 15 one-byte values and the meta byte: 16 value bytes; 30 qualifier bytes
        last = [sec_row(T0, list(range(0, 150, 10)), list(range(1, 16)))]
    else:                        # 8 float32 values and the meta byte: 33 value bytes; 16 qualifier bytes
        last = quarter_points(rng, T0 + np.arange(8) * 60).rows()
    series.append(last)
    n = len(series)
    a = synth.from_series(series, [0] * n)
    ids = scatter_ids(n, 4, excl_every=0, ungrouped=())
    ids[11:17] = 2                                       # the fifty-row series side by side: 300 one-word rows
    ids[n - 1] = NONE                                    # the ungrouped series is the last in descriptor order
    assert EXCL not in ids and list(ids).count(NONE) == 1
    end = T0 + 50 * H
    # (the series' timestamps differ: aggregators that do not interpolate keep the sums order-free)
    queries = [dsq(T0, end, "zimsum", "sum", 600000), dsq(T0, end, "mimmax", "max", 3600000)]
    eng.load(a)
    eng.regroup(ids)
    # the append replaces the last row of six series by itself: their old copies are dead bytes
    repl = [0, 3, 5, 7, 9, 12]
    d = synth.from_series([[series[i][-1]] for i in repl], [0] * len(repl))
    ainfo = eng.append(d, repl, np.zeros(len(repl)))
    al = lambda x: (len(x) + 15) & ~15   # noqa: E731
    assert ainfo.rows_replaced == len(repl)
    assert (ainfo.qual_dead, ainfo.val_dead) == (sum(al(series[i][-1][1]) for i in repl), sum(al(series[i][-1][2]) for i in repl))
    m = merge_batches(with_ids(a, ids), d, repl, np.zeros(len(repl)))
    info, _, t = check_trim(eng, m, 0, 0, queries, f"geometry {tail}", loaded=True)
    assert info.rows_evicted == 0 and info.series_emptied == 0 and info.rows_reindexed == 0
    assert (info.qual_reclaimed, info.val_reclaimed) == (ainfo.qual_dead, ainfo.val_dead)
    lastq, lastv = len(last[-1][1]), len(last[-1][2])
    assert (lastq % 16, lastv % 16) == ((14, 0) if tail == "exact" else (0, 1))


# ---- the cause of a k_recede flag evicted ---------------------------------------------------------
@gpu
@pytest.mark.parametrize("opts", [{}, {"INDEX_FUSED": 0}, {"INDEX_GENERIC": 1}], ids=["default", "unfused", "generic"])
@PACKS
def test_recede_cause_evicted(eng, pack, opts):
    """Hour 0's row ends with an offset past the hour (3700 s), so hour 1's row [10, 20, 30] --
    regular in itself -- is flagged by k_recede.  With hour 0 gone the flag has lost its cause."""
    from opentsdb_amd import engine
    rows = [
        [sec_row(T0, [0, 600, 1200, 3700], [1, 2, 3, 4]), sec_row(T0 + H, [10, 20, 30], [9, 10, 11])],
        [sec_row(T0, [0, 900], [5, 6]), sec_row(T0 + H, [100, 40, 900], [14, 15, 16])],       # unsorted in itself
        [sec_row(T0, [0, 100], [7, 8]), sec_row(T0 + H, [5, 3700], [17, 18]), sec_row(T0 + 2 * H, [10, 50], [19, 20])],
    ]
    a = synth.from_series(rows, [0, 0, 0])
    queries = [dsq(T0, T0 + 3 * H, "sum", "sum", 60000), abi.new_query(T0, T0 + 3 * H - 1, "sum")]
    with engine.options(**opts):
        eng.load(a)
        flags = eng.debug_rows()[1]
        assert [bool(f & UNSORTED) for f in flags] == [False, True, False, True, False, False, True]
        assert eng.debug_regular()[0][1].tolist() == [0, 0]
        info, _, _ = check_trim(eng, a, T0 + H, pack, queries, f"recede {opts}", loaded=True)
        assert info.rows_reindexed >= 1
        eng.load(a)
        eng.trim(T0 + H, pack)
        flags = eng.debug_rows()[1]
        reg = eng.debug_regular()[0]
    # series 0: hour 1; series 1: hour 1 (its own flag stays); series 2: hours 1 and 2 (hour 1 still recedes past hour 2)
    assert [bool(f & UNSORTED) for f in flags] == [False, True, False, True]
    assert reg[0].tolist() == [10, 10] and reg[1].tolist()[1] == 0 and reg[3].tolist()[1] == 0


# ---- with regroup and append ----------------------------------------------------------------------
@gpu
def test_excluded_series_are_trimmed_and_packed(eng):
    rng = np.random.default_rng(13)
    n = 9
    pts = [quarter_points(rng, T0 + np.arange(0, 3 * H, 30)) if s % 2 else int_points(rng, T0 + np.arange(0, 3 * H, 30), -100, 30000)
           for s in range(n)]
    a = synth.from_series([p.rows() for p in pts], [0] * n)
    ids = np.array([1, EXCL, 0, 0, EXCL, 1, NONE, 0, EXCL], np.int32)
    end = T0 + 3 * H
    queries = [dsq(T0, end, "sum", "sum", 60000), dsq(T0, end, "none", "sum", 600000)]
    eng.load(a)
    eng.regroup(ids)
    info, _, _ = check_trim(eng, with_ids(a, ids), T0 + H, 0, queries, "with exclusions", loaded=True)
    assert info.rows_evicted == n
    # the excluded series' rows went too: everything visible again equals a fresh load of the trimmed batch
    eng.load(a)
    eng.regroup(ids)
    eng.trim(T0 + H, 0)
    qoff, voff = eng.debug_layout()
    assert len(qoff) == 2 * n                            # every loaded row is in the packed layout
    ids2 = np.array([0, 1, 2, 0, 1, 2, 0, NONE, 1], np.int32)
    eng.regroup(ids2)
    got = state(eng, queries)
    rb, _ = restricted(trim_batch(a, T0 + H), ids2)
    for i, (q, g) in enumerate(zip(queries, got[0])):
        assert_groups_match(g, want_of(rb, q), agg_name(q), tol=0.0, ctx=f"readmitted q{i}")
    eng.load(rb)
    same_state(got, state(eng, queries), queries, "readmitted")


@gpu
def test_sliding_window(eng):
    """Load three hours (the last one partial), then twice: append the next hour (the live row
    replaced) and trim the oldest hour with a pack."""
    rng = np.random.default_rng(21)
    n = 8
    pts = [quarter_points(rng, T0 + np.arange(0, 6 * H, 30)) for _ in range(n)]
    gids = [s % 2 for s in range(n)]
    cur = synth.from_series([p.rows(None, T0 + 2 * H + 1800) for p in pts], gids)
    eng.load(cur)
    for k in (3, 4):
        lo, hi = T0 + (k - 2) * H, T0 + k * H + 1800
        queries = [dsq(lo - H, hi, "sum", "sum", 60000), dsq(lo, hi, "max", "max", 60000)]
        dd = synth.from_series([p.rows(T0 + (k - 1) * H, hi) for p in pts], gids)
        ainfo = eng.append(dd, np.arange(n), np.zeros(n))
        assert (ainfo.rows_added, ainfo.rows_replaced) == (n, n)
        cur = merge_batches(cur, dd, np.arange(n), np.zeros(n))
        for i, q in enumerate(queries):
            assert_groups_match(eng.run(q), O.run_query(cur, q), agg_name(q), tol=0.0, ctx=f"hour {k} appended q{i}")
        info = eng.trim(lo, 0)
        cur = trim_batch(cur, lo)
        assert (info.rows_evicted, info.packed, info.qual_dead, info.val_dead) == (n, 1, 0, 0)
        assert info.qual_reclaimed >= ainfo.qual_dead and info.val_reclaimed >= ainfo.val_dead
        for i, q in enumerate(queries):
            assert_groups_match(eng.run(q), O.run_query(cur, q), agg_name(q), tol=0.0, ctx=f"hour {k} trimmed q{i}")
        check_layout(eng, f"hour {k}")
    want = synth.from_series([p.rows(T0 + 2 * H, T0 + 4 * H + 1800) for p in pts], gids)
    batches_equal(cur, want)
    got = state(eng, queries)
    eng.load(cur)
    same_state(got, state(eng, queries), queries, "sliding window")


@gpu
@PACKS
def test_append_onto_a_series_the_trim_emptied(eng, pack):
    rng = np.random.default_rng(8)
    n = 6
    ts = T0 + np.arange(0, 3 * H, 60)
    pts = [int_points(rng, ts, -1000, 1000) for _ in range(n)]
    pts[2] = int_points(rng, np.concatenate([ts[ts < T0 + H], ts[ts >= T0 + 2 * H + 600]]), -1000, 1000)
    gids = [0, 1, 0, 1, NONE, 0]
    cut = T0 + 2 * H + 600
    a = synth.from_series([p.rows(None, cut) for p in pts], gids)
    end = T0 + 3 * H
    queries = [dsq(T0, end, "sum", "sum", 600000), dsq(T0, end, "first", "sum", 600000)]
    info, _, t = check_trim(eng, a, T0 + H, pack, queries, "emptying")
    assert info.series_emptied == 1 and int(t.series_row_ptr[3] - t.series_row_ptr[2]) == 0
    eng.load(a)
    eng.trim(T0 + H, pack)
    d = synth.from_series([p.rows(T0 + 2 * H, None) for p in pts], gids)
    ainfo, _, m = check_append(eng, t, d, np.arange(n), np.zeros(n), queries, "onto the emptied series", loaded=True)
    assert ainfo.rows_replaced == n - 1 and ainfo.rows_added == 1
    batches_equal(m, synth.from_series([p.rows(T0 + H, None) for p in pts], gids))


# ---- edges --------------------------------------------------------------------------------------------
@gpu
@PACKS
def test_edges(eng, pack):
    rng = np.random.default_rng(41)
    n = 5
    pts = [int_points(rng, T0 + np.arange(0, 3 * H, 300), 0, 1000) for _ in range(n)]
    gids = [0, 1, 0, 1, NONE]
    a = synth.from_series([p.rows() for p in pts], gids)
    end = T0 + 4 * H
    queries = [dsq(T0, end, "sum", "sum", 600000), dsq(T0, end, "none", "sum", 600000)]
    # a cutoff below every base, and none at all: nothing goes
    for cutoff in (T0, T0 - 5, 0, -7):
        info, _, _ = check_trim(eng, a, cutoff, pack, queries, f"no-op {cutoff}")
        assert info.rows_evicted == 0 and info.series_emptied == 0 and info.packed == (pack == 0)
    # twice is once with the larger cutoff
    eng.load(a)
    eng.trim(T0 + 2 * H, pack)
    check_trim(eng, trim_batch(a, T0 + 2 * H), T0 + H, pack, queries, "a smaller cutoff afterwards", loaded=True)
    eng.load(a)
    eng.trim(T0 + H, pack)
    check_trim(eng, trim_batch(a, T0 + H), T0 + 2 * H, pack, queries, "a larger cutoff afterwards", loaded=True)
    # a cutoff beyond every row: every series stays, without rows
    eng.load(a)
    for q in queries:
        eng.run(q)
    info = eng.trim(T0 + 9 * H, pack)
    assert (info.rows_evicted, info.series_emptied) == (a.n_rows, n) and eng.n_series() == n
    assert sizes(eng) == (n, 0, 0, 0)
    assert all(len(eng.run(q)) == 0 for q in queries)     # no group
    np.testing.assert_array_equal(eng.resident_groups(), resident_order(gids))
    empty = trim_batch(a, T0 + 9 * H)
    d = synth.from_series([p.rows(T0 + 2 * H, None) for p in pts], gids)
    check_append(eng, empty, d, np.arange(n), np.zeros(n), queries, "onto the emptied batch", loaded=True)
    # an empty load
    eng.load(synth.from_series([], []))
    info = eng.trim(T0, pack)
    assert info.rows_evicted == 0 and info.packed == 0


# ---- load_cells: a row whose compaction fails ---------------------------------------------------
@gpu
@PACKS
def test_load_cells_compaction_error(eng, pack):
    from opentsdb_amd.engine import EngineError
    rng = np.random.default_rng(11)
    good = [int_points(rng, T0 + np.arange(0, 3 * H, 60), 0, 1000) for _ in range(3)]
    q1 = struct.pack(">H", (10 << 4) | 0)
    q2 = struct.pack(">H", (20 << 4) | 0)
    cells = lambda rows: [(b, [(q, v, None)]) for b, q, v in rows]   # noqa: E731
    # series 1's middle row fails to compact: a second twice, with another value
    bad_row = (T0 + H, [(q1, b"\x01", None), (q1 + q2, b"\x02\x03\x00", None)])
    series = [cells(good[0].rows()), cells(good[1].rows(None, T0 + H)) + [bad_row] + cells(good[1].rows(T0 + 2 * H, None)),
              cells(good[2].rows())]
    q = dsq(T0, T0 + 3 * H, "sum", "sum", 600000)
    eng.load_cells(abi.HostCellBatch.from_rows(series, [0, 0, 1]))
    with pytest.raises(EngineError) as e0:
        eng.run(q)
    assert e0.value.java == "IllegalDataException"
    info = eng.trim(T0 + H, pack)                        # the bad row stays
    assert info.rows_evicted > 0
    with pytest.raises(EngineError) as e1:
        eng.run(q)
    assert (e1.value.code, str(e1.value)) == (e0.value.code, str(e0.value))
    info = eng.trim(T0 + 2 * H, pack)                    # the bad row goes
    assert info.rows_evicted > 0
    want = O.run_query(synth.from_series([p.rows(T0 + 2 * H, None) for p in good], [0, 0, 1]), q)
    assert_groups_match(eng.run(q), want, "sum", tol=0.0, ctx="bad row evicted")


# ---- rollup / pre-aggregate cells ---------------------------------------------------------------
@gpu
def test_rollup_and_preagg_cells(eng):
    from opentsdb_amd import engine
    rng = np.random.default_rng(31)
    pts = [quarter_points(rng, T0 + np.arange(0, 3 * H, 300)) for _ in range(6)]
    a = synth.from_series([p.rows() for p in pts], [0, 0, 1, 1, 2, NONE])
    iv = engine.rollup_interval("10m", "1d")
    end = T0 + 3 * H
    eng.load(a)
    old = eng.rollup(iv, T0, end, FUNCS)
    assert len(old) and eng.preagg_run(iv, T0, end, "sum", FUNCS)[0]
    eng.trim(T0 + H)
    ser = np.full(len(old), -7, np.int32)
    voff = np.full(len(old) + 1, 2 ** 63, np.uint64)
    assert engine.lib().tsdbhip_rollup_download(eng.ctx, ser.ctypes.data, None, None, voff.ctypes.data, None) == 0
    assert voff[0] == 0 and (ser == -7).all()
    assert resident_cells(eng) == 0
    cells = eng.rollup(iv, T0, end, FUNCS)
    pre = eng.preagg(iv, T0, end, "sum", FUNCS)
    assert 0 < len(cells) < len(old) and len(pre)
    eng.load(trim_batch(a, T0 + H))
    fresh = eng.rollup(iv, T0, end, FUNCS)
    for name in ("series", "base_time", "qualifier", "val_off", "value"):
        np.testing.assert_array_equal(getattr(cells, name), getattr(fresh, name), err_msg=name)
    fpre = eng.preagg(iv, T0, end, "sum", FUNCS)
    for name in ("func_index", "group", "base_time", "qual_off", "qualifier", "val_off", "value"):
        np.testing.assert_array_equal(getattr(pre, name), getattr(fpre, name), err_msg=name)


# ---- refusals --------------------------------------------------------------------------------------
def trim_code(e, cutoff, pack):
    from opentsdb_amd import engine
    return engine.lib().tsdbhip_trim(e.ctx, cutoff, pack, C.byref(abi.TrimInfo()))


@gpu
def test_refusals_leave_the_batch(eng):
    from opentsdb_amd import engine
    from opentsdb_amd.rollup_read import make_rollup_batch
    rng = np.random.default_rng(41)
    pts = [int_points(rng, T0 + np.arange(0, 3 * H, 300), 0, 1000) for _ in range(5)]
    a = synth.from_series([p.rows() for p in pts], [0, 1, 0, 1, NONE])
    NI, IA = abi.TSDB_E_NOT_IMPLEMENTED, abi.TSDB_E_ILLEGAL_ARGUMENT
    q = dsq(T0, T0 + 3 * H, "sum", "sum", 600000)
    eng.load(a)
    before = eng.run(q)
    assert trim_code(eng, T0 + H, 101) == IA
    identical(before, eng.run(q), "pack_dead_pct above 100")
    assert sizes(eng)[1] == a.n_rows
    iv = engine.rollup_interval("10m", "1d")
    cell = (struct.pack(">H", (0 << 4) | 0x7), struct.pack(">q", 5))
    eng.load_rollup(make_rollup_batch([(None, [(T0, [cell], [])])], [0], iv, False))
    assert trim_code(eng, T0 + H, 0) == NI
    eng.load_shard(a, engine.SHARD_SPANS, 0, a.n_series)
    before = eng.run(q)
    for pack in (NO_PACK, 0):
        assert trim_code(eng, T0 + H, pack) == NI
    identical(before, eng.run(q), "shard batch untouched")
    md = engine.Engine(devices=[0, 0])
    try:
        md.load(a)
        before = md.run(q)
        for pack in (NO_PACK, 0):
            assert trim_code(md, T0 + H, pack) == NI
        assert engine.lib().tsdbhip_debug_layout(md.ctx, None, None) == NI
        identical(before, md.run(q), "multi-device context untouched")
    finally:
        md.close()


# ---- ResidentSpans end to end --------------------------------------------------------------------
@gpu
def test_resident_spans_extend_and_trim_equal_tsdb_query(eng):
    from opentsdb_amd.query import ResidentSpans
    from tests.test_append_cpu import growing_store
    from tests.test_regroup_cpu import END, METRIC, QUERIES, START, query
    cut = START + 2 * 3600 + 1500
    st, full = growing_store(cut)
    new_start, new_end = START + 3600, END + 7200
    want = {}
    for i, tags in enumerate(QUERIES):
        q = query(full, tags, start=new_start, end=new_end - 1)
        q.runner = eng.run_batch
        want[i] = q.run()
    rs = ResidentSpans(st, METRIC, START, START + 3 * 3600, engine=eng)
    rs.run(query(st, {"host": "*"}, start=START, end=START + 3 * 3600 - 1))     # the old state over the old range
    st.rows = full.rows
    rs.extend(new_end)
    info = rs.trim(new_start, pack_dead_pct=0)
    assert info.rows_evicted == 11 and info.series_emptied == 1 and info.packed == 1
    for i, tags in enumerate(QUERIES):
        got = rs.run(query(st, tags, start=new_start, end=new_end - 1))
        exp = want[i]
        assert len(got) == len(exp), tags
        by = {d.group_key: d for d in got}
        for d in exp:
            g = by[d.group_key]
            for name in ("ts", "bits", "is_int"):
                np.testing.assert_array_equal(getattr(g, name), getattr(d, name), err_msg=f"{tags} {name}")
    with pytest.raises(ValueError, match="outside the resident range"):
        rs.run(query(st, {"host": "*"}, start=START, end=new_end - 1))
