"""GPU parity of tsdbhip_remove (k_remove.hip): rows removed from anywhere in the resident batch by
(series, base-time range) and row-less series retired, without a reload.

The expectation never comes from the engine: after load(A) + remove(R) the context must answer as a
fresh load of remove_batch(A, R, drop_empty) would (tests/remove_util.py, checked against stores
built from full point lists in tests/test_remove_cpu.py).  Every case first queries the OLD state,
removes, compares every query with the oracle over the remaining batch restricted to its visible
series bit for bit (tol = 0.0), and then compares results, debug_rows(), debug_regular()'s array,
download() and the batch sizes array for array with the same engine after a fresh load of that
batch.  After a pack the blob offsets are checked against the scan of the aligned lengths.

Inputs are order-free -- integers, or multiples of 0.25 below 2^20 -- so the default unordered
path must equal the oracle to the bit."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import pytest

from opentsdb_amd import abi, synth
from oracle import oracle as O
from tests.append_util import batches_equal, int_points, merge_batches, quarter_points, with_ids
from tests.remove_util import remove_batch
from tests.test_gpu_append import same_state, sec_row, sizes, state
from tests.test_gpu_parity import assert_groups_match
from tests.test_gpu_preagg import FUNCS, resident_cells
from tests.test_gpu_regroup import agg_name, dsq, identical, resident_order, restricted, want_of
from tests.test_gpu_trim import check_layout, class_store
from tests.trim_util import trim_batch

gpu = pytest.mark.gpu

T0 = 1356998400
H = 3600
EXCL = abi.GROUP_EXCLUDED
NONE = abi.GROUP_NONE
NO_PACK = abi.TRIM_NO_PACK
UNSORTED = 0x100000
ALL = (0, 1 << 32)
PACKS = pytest.mark.parametrize("pack", [NO_PACK, 0], ids=["nopack", "pack"])
GATHER_GRID_WORDS = 1024 * 256   # k_remove.hip: REMOVE_MAX_BLOCKS blocks of REMOVE_BLOCK one-word threads
DROPS = pytest.mark.parametrize("drop", [False, True], ids=["keep", "drop"])


@pytest.fixture(scope="module")
def eng():
    from opentsdb_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def hour(k):
    return (T0 + k * H, T0 + (k + 1) * H)


def rows_hit(a, ranges):
    """Rows of `a` each range covers."""
    ser = np.repeat(np.arange(a.n_series), np.diff(a.series_row_ptr))
    base = a.row_base_time[:a.n_rows].astype(np.int64)
    return [int(np.count_nonzero((ser == i) & (base >= lo) & (base < hi))) for i, lo, hi in ranges]


def check_remove(eng, a, ranges, drop, pack, queries, ctx, loaded=False):
    """One case.  `a` carries the PRESENT ids of the resident series (GROUP_EXCLUDED included, when
    the caller has regrouped).  Returns (info, results, remaining batch, new_index)."""
    if not loaded:
        eng.load(a)
    for q in queries:
        eng.run(q)                                   # the old state
    info, new_index = eng.remove(ranges, drop, pack)
    t, want_index = remove_batch(a, ranges, drop)
    np.testing.assert_array_equal(new_index, want_index, err_msg=f"{ctx} new_index")
    rb, kept = restricted(t, t.group_id)
    assert eng.n_series() == len(kept), ctx
    left = np.diff(remove_batch(a, ranges, False)[0].series_row_ptr)
    assert info.rows_removed == a.n_rows - t.n_rows, ctx
    assert info.series_emptied == int(np.count_nonzero((np.diff(a.series_row_ptr) > 0) & (left == 0))), ctx
    assert info.series_dropped == (int(np.count_nonzero(left == 0)) if drop else 0), ctx
    assert info.ranges_empty == sum(1 for h in rows_hit(a, ranges) if h == 0), ctx
    got = state(eng, queries)
    reg = eng.debug_regular()[0]
    for i, (q, g) in enumerate(zip(queries, got[0])):
        assert_groups_match(g, want_of(rb, q), agg_name(q), tol=0.0, ctx=f"{ctx} q{i} vs oracle")
    np.testing.assert_array_equal(got[4], resident_order(rb.group_id))
    assert got[3] == (rb.n_series, rb.n_rows, int(rb.row_qual_off[-1]), int(rb.row_val_off[-1])), ctx
    if pack == 0:
        assert info.qual_dead == 0 and info.val_dead == 0, ctx
        if info.packed:
            check_layout(eng, ctx)
    elif pack == NO_PACK:
        assert info.packed == 0 and info.qual_reclaimed == 0 and info.val_reclaimed == 0, ctx
    eng.load(rb)
    same_state(got, state(eng, queries), queries, ctx)
    np.testing.assert_array_equal(reg, eng.debug_regular()[0], err_msg=f"{ctx} debug_regular")
    return info, got[0], t, new_index


def small_store(seed=5, n=8, hours=4, gids=None):
    """n series of `hours` hour rows (12 integers a row); series 5 never had a row."""
    rng = np.random.default_rng(seed)
    pts = [int_points(rng, T0 + np.arange(0, hours * H, 300), 0, 1000) for _ in range(n)]
    series = [p.rows() for p in pts]
    if n > 5:
        series[5] = []
    gids = [0, 1, 2, 0, 1, 2, NONE, 3, 0, 1, 2, 0][:n] if gids is None else gids
    return synth.from_series(series, gids)


QS = [dsq(T0, T0 + 4 * H, "sum", "sum", 600000), dsq(T0, T0 + 4 * H, "none", "sum", 600000)]

PLACEMENTS = {
    "first": [(0, *hour(0))],
    "middle": [(1, *hour(1)), (2, T0 + 2 * H, T0 + 2 * H + 1)],
    "last": [(3, *hour(3))],
    "every_row": [(4, *ALL), (7, T0, T0 + 4 * H)],
    "two_disjoint": [(0, *hour(0)), (0, *hour(2)), (6, *hour(3)), (6, *hour(1))],
    "overlapping_repeated": [(1, T0, T0 + 2 * H), (1, T0 + H, T0 + 3 * H), (1, T0 + H, T0 + 3 * H), (2, *hour(1)), (2, *hour(1)),
                             (3, *ALL), (3, *hour(2))],
    "between_and_past": [(0, T0 + 1, T0 + H), (0, T0 + 4 * H, T0 + 9 * H), (1, T0 + 2 * H, T0 + 2 * H), (2, 0, T0),
                         (3, *hour(1))],
    "from_is_to": [(0, T0, T0), (1, T0 + H, T0 + H), (2, 0, 0)],
    "rowless_series": [(5, *ALL), (5, *hour(1)), (4, *hour(0))],
    "reverse_order": [(7, *hour(3)), (6, *hour(0)), (4, *hour(2)), (3, *hour(1)), (1, *hour(1)), (0, *hour(0))],
}


@gpu
@DROPS
@PACKS
@pytest.mark.parametrize("place", list(PLACEMENTS))
def test_placements(eng, place, pack, drop):
    a = small_store()
    ranges = PLACEMENTS[place]
    info, _, t, _ = check_remove(eng, a, ranges, drop, pack, QS, f"{place} {pack} {drop}")
    if place == "from_is_to":
        assert info.rows_removed == 0 and info.ranges_empty == 3
    if place == "between_and_past":
        assert info.rows_removed == 1 and info.ranges_empty == 4
    if place == "every_row":
        assert info.series_emptied == 2 and t.n_series == (5 if drop else 8)   # (series 5 goes with them)
    # idempotent: the same ranges once more, in the new numbering, remove nothing
    nx = remove_batch(a, ranges, drop)[1]
    again = [(int(nx[i]), lo, hi) for i, lo, hi in ranges if nx[i] >= 0]
    eng.load(t)
    before = state(eng, QS)
    info2, idx2 = eng.remove(again, drop, NO_PACK)
    assert (info2.rows_removed, info2.series_dropped, info2.ranges_empty) == (0, 0, len(again))
    np.testing.assert_array_equal(idx2, np.arange(t.n_series))
    same_state(before, state(eng, QS), QS, f"{place} again")


@gpu
@PACKS
def test_two_calls_equal_the_union(eng, pack):
    a = small_store()
    r1, r2 = PLACEMENTS["two_disjoint"], PLACEMENTS["overlapping_repeated"]
    eng.load(a)
    eng.remove(r1, False, pack)
    eng.remove(r2, True, pack)
    got = state(eng, QS)
    reg = eng.debug_regular()[0]
    check_remove(eng, a, r1 + r2, True, pack, QS, "the union")   # (leaves the fresh load of what remains)
    same_state(got, state(eng, QS), QS, "two calls")
    np.testing.assert_array_equal(reg, eng.debug_regular()[0])


# ---- row classes at tile size 1 -------------------------------------------------------------------
@gpu
@PACKS
@pytest.mark.parametrize("keep_one", [False, True], ids=["middle", "all_but_one"])
@pytest.mark.parametrize("name", ["short_f32", "short_int", "rows", "walker", "mixed"])
def test_row_classes(eng, name, keep_one, pack):
    pts, _, end = class_store(name)
    a = synth.from_series([p.rows() for p in pts], [i % 3 for i in range(len(pts))])
    bases = np.unique(a.row_base_time[:a.n_rows]).astype(np.int64)
    mid = int(bases[len(bases) // 2])
    gone = [b for b in bases if b != mid] if keep_one else [mid]
    ranges = [(s, int(b), int(b) + 1) for s in range(len(pts)) for b in gone]
    queries = [dsq(T0, end, "sum", "sum", 60000), dsq(T0, end, "max", "max", 60000), abi.new_query(T0, end - 1, "sum")]
    if name == "short_int":
        queries.append(dsq(T0, end, "p99", "avg", 60000))
    info, got, t, _ = check_remove(eng, a, ranges, False, pack, queries, f"{name} {keep_one} {pack}")
    assert info.rows_removed == len(pts) * len(gone) and info.series_emptied == 0 and info.ranges_empty == 0
    if keep_one:
        assert t.n_rows == len(pts)                  # one row a series: k_rows' class becomes k_short's


@gpu
def test_int16_copy_goes_with_its_rows(eng):
    """Integer (vle) series beside float ones: with every integer row removed and a pack, no kept
    row reads the int16 value copy and later queries equal the fresh load's."""
    rng = np.random.default_rng(17)
    pts = [int_points(rng, T0 + np.arange(0, 2 * H, 10), -100, 30000) if s % 2 else quarter_points(rng, T0 + np.arange(0, 2 * H, 10))
           for s in range(8)]
    a = synth.from_series([p.rows() for p in pts], [s % 2 for s in range(8)])
    queries = [dsq(T0, T0 + 2 * H, "sum", "sum", 60000), dsq(T0, T0 + 2 * H, "max", "max", 60000)]
    for drop in (False, True):
        info, _, t, _ = check_remove(eng, a, [(s, *ALL) for s in range(1, 8, 2)], drop, 0, queries, f"int16 {drop}")
        assert info.packed == 1 and info.series_emptied == 4 and info.series_dropped == (4 if drop else 0)


# ---- the cause of a k_recede flag removed ---------------------------------------------------------
def flag_rows():
    return [
        # hour 0 ends past the hour (3700 s): hour 1, regular in itself, is flagged
        [sec_row(T0, [0, 600, 1200, 3700], [1, 2, 3, 4]), sec_row(T0 + H, [10, 20, 30], [9, 10, 11])],
        # hour 0 reaches into hour 1 and hour 1 into hour 2: with hour 0 gone, hour 2's flag stays
        [sec_row(T0, [0, 3650], [5, 6]), sec_row(T0 + H, [20, 3700], [7, 8]), sec_row(T0 + 2 * H, [10, 50], [19, 20])],
        # hour 1 is unsorted in itself
        [sec_row(T0, [0, 900], [5, 6]), sec_row(T0 + H, [100, 40, 900], [14, 15, 16])],
        # the row after the flagged one goes: nothing is indexed again
        [sec_row(T0, [0, 3700], [1, 2]), sec_row(T0 + H, [10, 20], [3, 4]), sec_row(T0 + 2 * H, [100, 200], [5, 6])],
    ]


@gpu
@pytest.mark.parametrize("opts", [{}, {"INDEX_FUSED": 0}, {"INDEX_GENERIC": 1}], ids=["default", "unfused", "generic"])
@PACKS
def test_flags(eng, pack, opts):
    from opentsdb_amd import engine
    a = synth.from_series(flag_rows(), [0, 0, 1, 1])
    queries = [dsq(T0, T0 + 3 * H, "sum", "sum", 60000), abi.new_query(T0, T0 + 3 * H - 1, "sum")]
    flagged = lambda: [bool(f & UNSORTED) for f in eng.debug_rows()[1]]   # noqa: E731
    causes = [(0, *hour(0)), (1, *hour(0)), (2, *hour(0))]
    with engine.options(**opts):
        eng.load(a)
        #                    s0: h0    h1    s1: h0  h1    h2    s2: h0  h1    s3: h0  h1    h2
        assert flagged() == [False, True, False, True, True, False, True, False, True, False]
        assert eng.debug_regular()[0][1].tolist() == [0, 0]
        info, _, _, _ = check_remove(eng, a, causes, False, pack, queries, f"flags {opts}", loaded=True)
        # series 0's hour 1, series 1's hours 1 and 2, series 2's hour 1
        assert info.rows_reindexed == 4
        eng.load(a)
        info = eng.remove(causes[:1], False, pack)[0]
        assert info.rows_reindexed == 1
        eng.remove(causes[1:], False, pack)
        got = flagged()
        reg = eng.debug_regular()[0]
        eng.load(a)
        info = eng.remove([(3, *hour(2))], False, pack)[0]
        assert (info.rows_removed, info.rows_reindexed) == (1, 0)
        assert flagged() == [False, True, False, True, True, False, True, False, True]
    #              s0: h1  s1: h1  h2    s2: h1  s3: h0  h1    h2
    assert got == [False, False, True, True, False, True, False]
    assert reg[0].tolist() == [10, 10]        # the flag's cause is gone: the RegRow is back
    assert reg[2].tolist()[1] == 0 and reg[3].tolist()[1] == 0 and reg[5].tolist()[1] == 0


# ---- excluded series and regroup ------------------------------------------------------------------
@gpu
def test_excluded_series_and_regroup(eng):
    from opentsdb_amd.engine import EngineError
    rng = np.random.default_rng(13)
    n = 9
    pts = [quarter_points(rng, T0 + np.arange(0, 3 * H, 30)) if s % 2 else int_points(rng, T0 + np.arange(0, 3 * H, 30), -100, 30000)
           for s in range(n)]
    a = synth.from_series([p.rows() for p in pts], [0] * n)
    ids = np.array([1, EXCL, 0, 0, EXCL, 1, NONE, 3, EXCL], np.int32)
    end = T0 + 3 * H
    queries = [dsq(T0, end, "sum", "sum", 60000), dsq(T0, end, "none", "sum", 600000)]
    # rows of excluded series go, one of them entirely; so does the top group's only series
    ranges = [(1, *hour(1)), (4, *ALL), (7, *ALL), (0, *hour(0)), (8, *hour(2)), (6, *hour(1))]
    for drop in (False, True):
        eng.load(a)
        eng.regroup(ids)
        info, got, t, nx = check_remove(eng, with_ids(a, ids), ranges, drop, 0, queries, f"with exclusions {drop}", loaded=True)
        assert info.packed == 1 and info.series_emptied == 2
        assert [g for g, *_ in got[0]] == [0, 1]             # group 3 has no series with rows any more
        # n_groups itself: group 3's series is still there without the flag (four groups) and retired
        # with it (two), which the partials layout shows -- it refuses fewer global groups than local ones
        eng.load(a)
        eng.regroup(ids)
        eng.remove(ranges, drop, 0)
        assert eng.partials_layout(queries[0], 4).n_groups == 4
        if drop:
            assert eng.partials_layout(queries[0], 2).n_groups == 2
            with pytest.raises(EngineError):
                eng.partials_layout(queries[0], 1)
        else:
            with pytest.raises(EngineError) as e3:
                eng.partials_layout(queries[0], 3)
            assert e3.value.code == abi.TSDB_E_ILLEGAL_ARGUMENT
    assert t.group_id.tolist() == [1, EXCL, 0, 0, 1, NONE, EXCL] and nx.tolist() == [0, 1, 2, 3, -1, 4, 5, -1, 6]
    # the kept rows of the excluded series are there: a regroup in the NEW numbering readmits them
    eng.load(a)
    eng.regroup(ids)
    eng.remove(ranges, True, 0)
    assert len(eng.debug_layout()[0]) == t.n_rows            # every loaded row is in the packed layout
    with pytest.raises(EngineError) as e:
        eng.regroup(np.zeros(n, np.int32))                   # N ids: refused
    assert e.value.code == abi.TSDB_E_ILLEGAL_ARGUMENT
    ids2 = np.array([0, 1, 2, 0, 1, NONE, 1], np.int32)
    eng.regroup(ids2)
    got = state(eng, queries)
    rb, _ = restricted(t, ids2)
    for i, (q, g) in enumerate(zip(queries, got[0])):
        assert_groups_match(g, want_of(rb, q), agg_name(q), tol=0.0, ctx=f"readmitted q{i}")
    eng.load(rb)
    same_state(got, state(eng, queries), queries, "readmitted")


# ---- sequences --------------------------------------------------------------------------------------
@gpu
def test_sequence_of_edits(eng):
    """load / append / remove(drop) / upsert in the new numbering / trim(pack) / remove / regroup, each
    step against a fresh load of the host-side batch."""
    rng = np.random.default_rng(23)
    n = 8
    pts = [quarter_points(rng, T0 + np.arange(0, 5 * H, 300)) for _ in range(n)]
    gids = [0, 1, 2, 0, 1, 2, NONE, 0]
    end = T0 + 5 * H
    queries = [dsq(T0, end, "sum", "sum", 600000), dsq(T0, end, "max", "max", 600000)]

    from opentsdb_amd.engine import Engine
    fresh = Engine(0)                                        # the fresh loads: the edited context goes on as it is

    def verify(cur, ctx):
        rb, _ = restricted(cur, cur.group_id)
        got = state(eng, queries)
        for i, (q, g) in enumerate(zip(queries, got[0])):
            assert_groups_match(g, want_of(rb, q), agg_name(q), tol=0.0, ctx=f"{ctx} q{i}")
        fresh.load(rb)
        same_state(got, state(fresh, queries), queries, ctx)
        np.testing.assert_array_equal(eng.debug_regular()[0], fresh.debug_regular()[0], err_msg=f"{ctx} debug_regular")

    try:
        _sequence(eng, verify, pts, gids, n)
    finally:
        fresh.close()


def _sequence(eng, verify, pts, gids, n):
    cur = synth.from_series([p.rows(None, T0 + 3 * H) for p in pts], gids)
    eng.load(cur)
    d = synth.from_series([p.rows(T0 + 3 * H, T0 + 4 * H) for p in pts], gids)
    eng.append(d, np.arange(n), np.zeros(n))
    cur = merge_batches(cur, d, np.arange(n), np.zeros(n))
    verify(cur, "appended")
    ranges = [(2, *ALL), (5, *ALL), (0, *hour(1)), (7, *hour(3))]
    info, nx = eng.remove(ranges, True, NO_PACK)
    cur, want_nx = remove_batch(cur, ranges, True)
    np.testing.assert_array_equal(nx, want_nx)
    assert info.series_dropped == 2 and cur.n_series == 6
    verify(cur, "removed")
    # upsert in the NEW numbering: old series 3 is 2 now and gets its hour 4; old series 0 gets hour 1 back
    d = synth.from_series([pts[0].rows(T0 + H, T0 + 2 * H), pts[3].rows(T0 + 4 * H, None)], [0, 0])
    eng.upsert(d, [0, 2], [0, 0])
    cur = merge_batches(cur, d, [0, 2], [0, 0])
    verify(cur, "upserted")
    tinfo = eng.trim(T0 + H, 0)
    cur = trim_batch(cur, T0 + H)
    assert tinfo.packed == 1 and tinfo.rows_evicted == 6
    verify(cur, "trimmed")
    info, _ = eng.remove([(1, *hour(2)), (5, *hour(1))], False, 0)
    cur, _ = remove_batch(cur, [(1, *hour(2)), (5, *hour(1))], False)
    assert info.rows_removed == 2 and info.packed == 1
    verify(cur, "removed again")
    ids = np.array([2, 2, EXCL, 0, NONE, 1], np.int32)
    eng.regroup(ids)
    verify(with_ids(cur, ids), "regrouped")


@gpu
@PACKS
def test_remove_of_every_prefix_is_a_trim(eng, pack):
    a = small_store()
    cutoff = T0 + 2 * H
    eng.load(a)
    tinfo = eng.trim(cutoff, pack)
    want = state(eng, QS)
    wreg, wlay = eng.debug_regular()[0], eng.debug_layout()
    eng.load(a)
    info, _ = eng.remove([(s, 0, cutoff) for s in range(a.n_series)], False, pack)
    assert (info.rows_removed, info.series_emptied, info.packed) == (tinfo.rows_evicted, tinfo.series_emptied, tinfo.packed)
    assert (info.qual_dead, info.val_dead, info.qual_reclaimed, info.val_reclaimed) == \
        (tinfo.qual_dead, tinfo.val_dead, tinfo.qual_reclaimed, tinfo.val_reclaimed)
    same_state(state(eng, QS), want, QS, "remove as trim")
    np.testing.assert_array_equal(eng.debug_regular()[0], wreg)
    for x, y in zip(eng.debug_layout(), wlay):
        np.testing.assert_array_equal(x, y)


@gpu
def test_remove_undoes_an_inserting_upsert(eng):
    rng = np.random.default_rng(3)
    pts = [int_points(rng, T0 + np.arange(0, 3 * H, 300), 0, 1000) for _ in range(7)]
    gids = [0, 1, 0, 1, NONE, 2, 2]
    # resident: six series without their hour 1; the delta brings hour 1 and a seventh series (index 3)
    res = [s for s in range(7) if s != 3]
    a = synth.from_series([pts[s].rows(None, T0 + H) + pts[s].rows(T0 + 2 * H, None) for s in res], [gids[s] for s in res])
    d = synth.from_series([pts[s].rows(T0 + H, T0 + 2 * H) if s != 3 else pts[s].rows() for s in range(7)], gids)
    eng.load(a)
    want = state(eng, QS)
    wreg = eng.debug_regular()[0]
    uinfo = eng.upsert(d, np.arange(7), [s == 3 for s in range(7)])
    assert (uinfo.series_added, uinfo.rows_added, uinfo.rows_replaced) == (1, 9, 0)
    info, nx = eng.remove([(s, *hour(1)) for s in range(7) if s != 3] + [(3, *ALL)], True, NO_PACK)
    assert (info.rows_removed, info.series_dropped) == (9, 1) and nx.tolist() == [0, 1, 2, -1, 3, 4, 5]
    same_state(state(eng, QS), want, QS, "upsert undone")
    np.testing.assert_array_equal(eng.debug_regular()[0], wreg)


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
    # series 0 is retired and series 1 loses its first row: the bad row stays, in a renumbered series
    info, nx = eng.remove([(0, *ALL), (1, *hour(0))], True, pack)
    assert info.series_dropped == 1 and nx.tolist() == [-1, 0, 1]
    with pytest.raises(EngineError) as e1:
        eng.run(q)
    assert e1.value.code == e0.value.code and e1.value.java == "IllegalDataException"
    # the bad row goes, by its new index (it was never resident: the range covers no resident row)
    info, _ = eng.remove([(0, *hour(1))], False, pack)
    assert info.rows_removed == 0 and info.ranges_empty == 1
    want = O.run_query(synth.from_series([good[1].rows(T0 + 2 * H, None), good[2].rows()], [0, 1]), q)
    assert_groups_match(eng.run(q), want, "sum", tol=0.0, ctx="bad row removed")


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
    ranges = [(s, *hour(1)) for s in range(6)]
    eng.remove(ranges)
    assert resident_cells(eng) == 0
    cells = eng.rollup(iv, T0, end, FUNCS)
    pre = eng.preagg(iv, T0, end, "sum", FUNCS)
    assert 0 < len(cells) < len(old) and len(pre)
    eng.load(remove_batch(a, ranges)[0])
    fresh = eng.rollup(iv, T0, end, FUNCS)
    for name in ("series", "base_time", "qualifier", "val_off", "value"):
        np.testing.assert_array_equal(getattr(cells, name), getattr(fresh, name), err_msg=name)
    fpre = eng.preagg(iv, T0, end, "sum", FUNCS)
    for name in ("func_index", "group", "base_time", "qual_off", "qualifier", "val_off", "value"):
        np.testing.assert_array_equal(getattr(pre, name), getattr(fpre, name), err_msg=name)


# ---- every series retired ---------------------------------------------------------------------------
@gpu
@PACKS
def test_every_series_retired(eng, pack):
    """N' = 0: the context equals one that loaded the empty batch, and takes a regroup of no ids
    and an append of new series as that one does."""
    a = small_store()
    eng.load(a)
    for q in QS:
        eng.run(q)
    info, nx = eng.remove([(s, *ALL) for s in range(a.n_series)], True, pack)
    assert (info.rows_removed, info.series_emptied, info.series_dropped) == (a.n_rows, 7, 8)
    assert (nx == -1).all() and sizes(eng) == (0, 0, 0, 0) and info.packed == (pack == 0)
    got = state(eng, QS)
    assert all(len(r) == 0 for r in got[0])
    eng.load(synth.from_series([], []))
    same_state(got, state(eng, QS), QS, "every series retired")
    # the edited context goes on: no ids to regroup, then three new series
    eng.load(a)
    eng.remove([(s, *ALL) for s in range(a.n_series)], True, pack)
    eng.regroup(np.zeros(1, np.int32)[:0])               # (no ids, from a pointer that is not null)
    d = small_store(seed=9, n=3, gids=[1, 0, NONE])
    ainfo = eng.append(d, np.arange(3), np.ones(3))
    assert (ainfo.series_added, ainfo.rows_added) == (3, d.n_rows)
    got = state(eng, QS)
    reg = eng.debug_regular()[0]
    for i, (q, g) in enumerate(zip(QS, got[0])):
        assert_groups_match(g, want_of(d, q), agg_name(q), tol=0.0, ctx=f"appended to nothing q{i}")
    eng.load(d)
    same_state(got, state(eng, QS), QS, "appended to nothing")
    np.testing.assert_array_equal(reg, eng.debug_regular()[0])


# ---- no-op and refusals ---------------------------------------------------------------------------
def remove_code(e, ranges, flags=0, pack=NO_PACK, n=None, null=False):
    from opentsdb_amd import engine
    arr = (abi.RemoveRange * max(1, len(ranges)))(*[abi.RemoveRange(*r) for r in ranges])
    return engine.lib().tsdbhip_remove(e.ctx, None if null else C.cast(arr, C.c_void_p), len(ranges) if n is None else n,
                                       flags, pack, None, C.byref(abi.RemoveInfo()))


@gpu
def test_noop_changes_nothing(eng):
    a = small_store()
    eng.load(a)
    before = state(eng, QS)
    cnt, fused = eng.debug_index()
    lay = eng.debug_layout()
    info, nx = eng.remove([(0, T0 + 1, T0 + H), (3, T0 + 7 * H, 1 << 32), (5, *ALL)], False, NO_PACK)
    assert (info.rows_removed, info.series_emptied, info.series_dropped, info.ranges_empty, info.packed) == (0, 0, 0, 3, 0)
    np.testing.assert_array_equal(nx, np.arange(a.n_series))
    same_state(before, state(eng, QS), QS, "no-op")
    cnt2, fused2 = eng.debug_index()
    np.testing.assert_array_equal(cnt, cnt2)
    assert fused == fused2 and cnt.sum() > 0
    for x, y in zip(eng.debug_layout(), lay):
        np.testing.assert_array_equal(x, y)
    info, _ = eng.remove([], False, NO_PACK)
    assert info.rows_removed == 0 and info.qual_capacity > 0
    eng.load(synth.from_series([], []))
    info, nx = eng.remove([], True, 0)
    assert info.rows_removed == 0 and info.packed == 0 and len(nx) == 0


@gpu
def test_refusals_leave_the_batch(eng):
    from opentsdb_amd import engine
    from opentsdb_amd.rollup_read import make_rollup_batch
    a = small_store()
    NI, IA = abi.TSDB_E_NOT_IMPLEMENTED, abi.TSDB_E_ILLEGAL_ARGUMENT
    ok = [(0, *hour(1))]
    eng.load(a)
    before = state(eng, QS)
    reg, lay = eng.debug_regular()[0], eng.debug_layout()
    illegal = {
        "pack_dead_pct above 100": dict(ranges=ok, pack=101),
        "n_ranges below 0": dict(ranges=ok, n=-1),
        "null ranges": dict(ranges=ok, null=True),
        "series_index N": dict(ranges=[(a.n_series, *hour(1))]),
        "series_index -1": dict(ranges=ok + [(-1, *hour(1))]),
        "from_s above to_s": dict(ranges=ok + [(1, T0 + H, T0)]),
        "from_s below 0": dict(ranges=ok + [(1, -1, T0)]),
        "flag bit 1": dict(ranges=ok, flags=2),
        "flag bit 31": dict(ranges=ok, flags=abi.REMOVE_DROP_EMPTY | 0x80000000),
    }
    for ctx, kw in illegal.items():
        assert remove_code(eng, kw.pop("ranges"), **kw) == IA, ctx
        same_state(before, state(eng, QS), QS, ctx)           # each refusal leaves the batch as it was
        np.testing.assert_array_equal(reg, eng.debug_regular()[0], err_msg=ctx)
        for x, y in zip(eng.debug_layout(), lay):
            np.testing.assert_array_equal(x, y, err_msg=ctx)
    assert engine.lib().tsdbhip_remove(None, None, 0, 0, 0, None, None) == IA
    same_state(before, state(eng, QS), QS, "null context")

    def answers(e):
        """What each query gives: its groups, or the error it raises (a rollup batch refuses some)."""
        out = []
        for q in QS:
            try:
                out.append(e.run(q))
            except engine.EngineError as x:
                out.append(str(x))
        return out

    def unchanged(e, was, ctx):
        for i, (x, y) in enumerate(zip(was, answers(e))):
            if isinstance(x, str) or isinstance(y, str):
                assert x == y, f"{ctx} q{i}"
            else:
                identical(x, y, f"{ctx} q{i}")

    iv = engine.rollup_interval("10m", "1d")
    cell = (struct.pack(">H", (0 << 4) | 0x7), struct.pack(">q", 5))
    eng.load_rollup(make_rollup_batch([(None, [(T0, [cell], [])])], [0], iv, False))
    was = answers(eng)
    assert any(not isinstance(w, str) for w in was)          # (the rollup batch answers a query)
    for ranges, flags, pack in ((ok, 0, NO_PACK), (ok, 0, 0), ([], 1, 0)):
        assert remove_code(eng, ranges, flags=flags, pack=pack) == NI
        unchanged(eng, was, f"rollup batch {flags} {pack}")
    eng.load_shard(a, engine.SHARD_SPANS, 0, a.n_series)
    was, size = answers(eng), sizes(eng)
    for pack in (NO_PACK, 0):
        assert remove_code(eng, ok, pack=pack) == NI
        unchanged(eng, was, f"shard batch {pack}")
        assert sizes(eng) == size
    md = engine.Engine(devices=[0, 0])
    try:
        md.load(a)
        was = answers(md)
        for pack in (NO_PACK, 0):
            assert remove_code(md, ok, pack=pack) == NI
            unchanged(md, was, f"multi-device context {pack}")
    finally:
        md.close()


# ---- scale ----------------------------------------------------------------------------------------
@gpu
def test_scale(eng):
    """131 072 series of two one-point rows: one row of every third series and both rows of every
    fifth go, with drop_empty and a pack -- every scan's tile boundaries are crossed, and the 524 286
    destination words of the kept rows are twice the gather's grid (REMOVE_MAX_BLOCKS = 1024 blocks of
    256 one-word threads), so every thread takes the grid-stride loop's second turn.  The comparison
    is with a fresh load."""
    n = 131072
    rng = np.random.default_rng(7)
    nr = 2 * n
    offs = rng.integers(0, 3600, nr).astype(np.uint16) << 4
    qual = np.stack([(offs >> 8).astype(np.uint8), (offs & 0xFF).astype(np.uint8)], axis=1).reshape(-1)
    val = rng.integers(1, 100, nr).astype(np.uint8)
    a = abi.HostBatch(np.arange(n + 1, dtype=np.int64) * 2, np.tile(np.array([T0, T0 + H], np.uint32), n),
                      np.arange(nr + 1, dtype=np.uint64) * 2, np.arange(nr + 1, dtype=np.uint64), qual, val,
                      (np.arange(n) % 64).astype(np.int32))
    s = np.arange(n)
    third, fifth = s[s % 3 == 0], s[s % 5 == 0]
    ranges = np.concatenate([np.stack([third, np.full(len(third), T0 + H * (third % 2)), np.full(len(third), T0 + H * (third % 2) + 1)], 1),
                             np.stack([fifth, np.zeros(len(fifth), np.int64), np.full(len(fifth), 1 << 32)], 1)])
    ranges = [tuple(int(x) for x in r) for r in rng.permutation(ranges)]
    queries = [dsq(T0, T0 + 2 * H, "sum", "sum", 3600000)]
    eng.load(a)
    eng.run(queries[0])
    info, nx = eng.remove(ranges, True, 0)
    t, want_nx = remove_batch(a, ranges, True)
    np.testing.assert_array_equal(nx, want_nx)
    assert info.series_dropped == len(fifth) and info.rows_removed == a.n_rows - t.n_rows and info.packed == 1
    assert 3 * t.n_rows > GATHER_GRID_WORDS                  # the gather's grid-stride cap is crossed
    got = state(eng, queries)
    reg = eng.debug_regular()[0]
    check_layout(eng, "scale")
    eng.load(t)
    same_state(got, state(eng, queries), queries, "scale")
    np.testing.assert_array_equal(reg, eng.debug_regular()[0])


# ---- ResidentSpans end to end --------------------------------------------------------------------
@gpu
def test_resident_spans_delete_and_refresh_equal_tsdb_query(eng):
    from opentsdb_amd.query import ResidentSpans
    from tests.test_regroup_cpu import END, METRIC, QUERIES, START, make_store, query

    def compare(rs, st, ctx, ref_eng):
        for tags in QUERIES:
            q = query(st, tags, start=START, end=END - 1)
            q.runner = ref_eng.run_batch
            exp = q.run()
            got = rs.run(query(st, tags, start=START, end=END - 1))
            assert len(got) == len(exp), (ctx, tags)
            by = {d.group_key: d for d in got}
            for d in exp:
                g = by[d.group_key]
                for name in ("ts", "bits", "is_int"):
                    np.testing.assert_array_equal(getattr(g, name), getattr(d, name), err_msg=f"{ctx} {tags} {name}")

    from opentsdb_amd.engine import Engine
    ref_eng = Engine(0)                                      # TsdbQuery's own loads: the resident batch stays in `eng`
    try:
        _delete_and_refresh(eng, ref_eng, compare)
    finally:
        ref_eng.close()


def _delete_and_refresh(eng, ref_eng, compare):
    from opentsdb_amd.query import ResidentSpans
    from tests.test_regroup_cpu import END, METRIC, QUERIES, START, make_store, query
    st = make_store()
    rs = ResidentSpans(st, METRIC, START, END, engine=ref_eng)
    dq = query(st, QUERIES[1], start=START + H, end=START + 2 * H - 1)
    ref = query(st, QUERIES[1], start=START + H, end=START + 2 * H - 1)
    ref.runner = ref_eng.run_batch
    exp = ref.run()
    rs2 = ResidentSpans(st, METRIC, START, END, engine=eng)
    out, info = rs2.delete(dq)
    assert len(out) == len(exp) and info.rows_removed > 0     # the delete query returns what it deletes
    compare(rs2, st, "deleted", ref_eng)
    # rows leave the store behind the resident spans' back: refresh(remove_missing=True) follows
    gone = st.delete_rows(METRIC, START + 2 * H, START + 3 * H, lambda tags: True)
    assert gone
    rs2.refresh(START + 2 * H, START + 3 * H, remove_missing=True)
    compare(rs2, st, "refreshed", ref_eng)
    info = rs2.retire_empty()
    assert info.series_dropped == sum(1 for sk in rs.span_keys if sk not in rs2.span_keys)
    assert rs2.spans == st.scan(METRIC, START, END)
    compare(rs2, st, "retired", ref_eng)
