"""GPU parity of tsdbhip_put (k_put.hip): datapoint writes merged into the resident rows on the
device.

The expectation never comes from the engine: after load(A) + put(P) the context must answer as a
fresh load of tests/put_util.py::put_batch(A, P) would -- the store's encoders and the oracle's
CompactionQueue over [(resident cell)] + the puts, checked against MockStores built from the full
point lists in tests/test_put_cpu.py.  Every case follows tests/test_gpu_upsert.py's check_upsert:
it queries the OLD state, puts, compares every query with the oracle over the expected batch
restricted to its visible series bit for bit (tol = 0.0), compares results, debug_rows(),
download(), sizes, the resident order and debug_regular() with the same engine after a fresh load
of that batch, checks the info counters, and repeats everything under PUT_WALK=1, where no row
may take the tail route.  A refused put must leave the state as it was (same_state).

Inputs are order-free: integers, or multiples of 0.25 below 2^20; groups of several series have a
point in every bucket.  No case relies on equal HBase write timestamps."""
from __future__ import annotations

import struct

import numpy as np
import pytest

from opentsdb_amd import abi, synth
from oracle import oracle as O
from tests.append_util import batches_equal, quarter_points, with_ids
from tests.put_util import D, F, L, put_batch, store_batch
from tests.put_util import encode as put_util_encode
from tests.test_gpu_append import same_state, sec_row, sizes, state
from tests.test_gpu_parity import assert_groups_match
from tests.test_gpu_preagg import FUNCS, resident_cells
from tests.test_gpu_regroup import agg_name, dsq, identical, resident_order, restricted, want_of
from tests.test_put_cpu import (FIVE, LONG_EDGES, PLACEMENTS, SAME_QUALIFIER_IN_CELL, resident_row, size_case)

gpu = pytest.mark.gpu

T0 = 1356998400
H = 3600
EXCL = abi.GROUP_EXCLUDED
UNSORTED = 0x100000
IA, ID, NI = abi.TSDB_E_ILLEGAL_ARGUMENT, abi.TSDB_E_ILLEGAL_DATA, abi.TSDB_E_NOT_IMPLEMENTED


@pytest.fixture(scope="module")
def eng():
    from opentsdb_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def load_case(eng, a):
    """`a` carries the present ids; excluded series become so by a regroup after the load."""
    ids = np.asarray(a.group_id)
    if (ids == EXCL).any():
        eng.load(with_ids(a, np.where(ids == EXCL, 0, ids)))
        eng.regroup(ids)
    else:
        eng.load(a)


def std_queries(lo, hi):
    return [dsq(lo, hi, "sum", "sum", 60000), dsq(lo, hi, "max", "max", 60000), abi.new_query(lo, hi - 1, "sum")]


def span_of(a, puts):
    ts = [int(b) for b in a.row_base_time] + [t // 1000 if t >> 32 else t for _, t, _, _ in puts]
    lo = min(ts) - min(ts) % H
    return lo, max(ts) - max(ts) % H + H


def put_code(eng, puts, fix):
    from opentsdb_amd.engine import EngineError
    try:
        return eng.put(puts, fix_duplicates=fix)
    except EngineError as e:
        return e.code


def check_put(eng, a, puts, fix, ctx, queries=None, tail=None, loader=load_case):
    """One case, routed and under PUT_WALK=1.  Returns (info, expectation); for a refusal (the
    expectation is an error code) (code, None)."""
    from opentsdb_amd import engine
    exp = put_batch(a, puts, fix)
    if queries is None:
        queries = std_queries(*span_of(a, puts))
    fresh = None
    first = None
    for walk in (False, True):
        with engine.options(PUT_WALK=1 if walk else -1):
            loader(eng, a)
            before = state(eng, queries)                     # the old state
            reg0 = eng.debug_regular()[0]
            info = put_code(eng, puts, fix)
            if isinstance(exp, int):
                assert info == exp, (ctx, walk, info)
                same_state(state(eng, queries), before, queries, f"{ctx} refused walk={walk}")
                np.testing.assert_array_equal(reg0, eng.debug_regular()[0])
                first = first or info
                continue
            assert not isinstance(info, int), (ctx, walk, info)
            got = state(eng, queries)
            reg = eng.debug_regular()[0]
        m = exp.batch
        rb, kept = restricted(m, m.group_id)
        assert eng.n_series() == len(kept), ctx
        if fresh is None:
            for i, (q, g) in enumerate(zip(queries, got[0])):
                assert_groups_match(g, want_of(rb, q), agg_name(q), tol=0.0, ctx=f"{ctx} q{i} vs oracle")
            np.testing.assert_array_equal(got[4], resident_order(rb.group_id))
            assert got[3] == (rb.n_series, rb.n_rows, int(rb.row_qual_off[-1]), int(rb.row_val_off[-1])), ctx
            eng.load(rb)
            fresh = state(eng, queries), eng.debug_regular()[0]
        same_state(got, fresh[0], queries, f"{ctx} walk={walk}")
        np.testing.assert_array_equal(reg, fresh[1], err_msg=f"{ctx} walk={walk} debug_regular")
        assert (info.points, info.points_shadowed, info.rows_added) == (len(puts), exp.shadowed, exp.added), (ctx, walk)
        assert info.rows_tail + info.rows_walked == exp.rewritten, (ctx, walk)
        assert info.kernel_ms >= 0.0
        if walk:
            assert info.rows_tail == 0 and info.rows_walked == exp.rewritten, ctx
        else:
            first = info
            if tail is not None:
                assert info.rows_tail == tail, (ctx, info.rows_tail, info.rows_walked)
    return first, (None if isinstance(exp, int) else exp)


# ---- 1. resident row sizes x puts a row ----------------------------------------------------------
@gpu
@pytest.mark.parametrize("where", ["spread", "tail"])
@pytest.mark.parametrize("k", [1, 2, 64, 65])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 3600])
def test_sizes_and_counts(eng, n, k, where):
    series, gids, puts = size_case(n, k, where)
    a = store_batch(series, gids)
    # (a one-datapoint row of a 2-byte qualifier is read with the single-datapoint fixups: walked)
    info, exp = check_put(eng, a, puts, False, f"n={n} k={k} {where}", tail=1 if where == "tail" and n > 1 else 0)
    assert exp.batch.n_rows == 1 and int(np.diff(exp.batch.row_qual_off)[0]) >= 2 * (n + k) and info.grew in (0, 1)


# ---- 2. placements ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fix", [False, True], ids=["nofix", "fix"])
@pytest.mark.parametrize("name", list(PLACEMENTS))
def test_placements(eng, name, fix):
    series, gids, puts = PLACEMENTS[name]
    a = store_batch(series, gids)
    tail = {"after_last": 1, "last_offsets": 1, "before_first": 0, "between": 0}.get(name)
    info, exp = check_put(eng, a, puts, fix, f"{name} fix={fix}", tail=tail)
    if name in ("equal_other_bytes", "second_and_ms_same_instant_other_bytes"):
        assert (info == ID) == (not fix)
    if name == "new_hours":
        assert (info.rows_added, info.rows_tail, info.rows_walked) == (3, 0, 0)
    if name == "zero_row_and_excluded":
        assert (info.rows_added, info.rows_walked) == (2, 1)
    if name == "same_qualifier_twice":
        assert info.points_shadowed == 1


@gpu
def test_the_compacted_column_deviation(eng):
    """The put's qualifier already sits in the resident cell: refused without the fix flag (the
    message names the series, the base and the ms offset), the put's value with it."""
    from opentsdb_amd import engine
    series, gids, puts = SAME_QUALIFIER_IN_CELL
    a = store_batch(series, gids)
    code, _ = check_put(eng, a, puts, False, "deviation")
    assert code == ID
    eng.load(a)
    assert put_code(eng, puts, False) == ID
    msg = engine.lib().tsdbhip_last_error().decode()
    assert "series 0" in msg and f"base {T0}" in msg and "ms_offset=300000" in msg
    info, exp = check_put(eng, a, puts, True, "deviation, fixed")
    assert bytes(exp.batch.val[:6]) == bytes([1, 2, 77, 4, 5, 0]) and info.rows_walked == 1


# ---- 3. values ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("where", ["tail", "between"])
def test_long_edges(eng, where):
    res = [(T0 + 600 * i, L, i) for i in range(3)]
    first = 1260 if where == "tail" else 60
    puts = [(0, T0 + first + 120 * j, L, v) for j, v in enumerate(LONG_EDGES)]
    qs = [dsq(T0, T0 + H, "max", "max", 60000), dsq(T0, T0 + H, "min", "min", 60000), abi.new_query(T0, T0 + H - 1, "sum")]
    info, exp = check_put(eng, store_batch([res], [0]), puts, False, f"long edges {where}", queries=qs, tail=int(where == "tail"))
    assert int(np.diff(exp.batch.row_val_off)[0]) == 3 + sum([2, 1, 1, 2, 2, 4, 2, 4, 4, 8, 4, 8, 8, 8]) + 1


@gpu
def test_float_against_double(eng):
    rng = np.random.default_rng(3)
    res = [(T0 + 60 * i, F, float(rng.integers(1, 1 << 20)) * 0.25) for i in range(30)]
    a = store_batch([res], [0])
    new = [(0, T0 + 1800 + 60 * j, D, float(rng.integers(1, 1 << 20)) * 0.25) for j in range(10)]
    info, _ = check_put(eng, a, new, False, "doubles behind floats", tail=1)
    mid = [(0, T0 + 30 + 60 * j, D, 0.25 * (j + 1)) for j in range(10)]
    check_put(eng, a, mid, False, "doubles between floats", tail=0)
    same = [(0, T0 + 60, D, res[1][2])]                     # the same number in eight bytes: other value bytes
    assert check_put(eng, a, same, False, "double onto float")[0] == ID
    info, exp = check_put(eng, a, same, True, "double onto float, fixed")
    assert info.rows_walked == 1 and exp.batch.row_val_off[-1] == 4 * 29 + 8 + 1


@gpu
@pytest.mark.parametrize("opts", [{}, {"INDEX_FUSED": 0}, {"INDEX_GENERIC": 1}], ids=["default", "unfused", "generic"])
@pytest.mark.parametrize("kind", ["int_into_float", "float_into_int"])
def test_class_change(eng, kind, opts):
    """Float32-only rows (no int16 value copy) gain 1-2-byte integers and the reverse: the rewritten
    rows change their index class, as tests/test_gpu_upsert.py's replaced rows do."""
    from opentsdb_amd import engine
    rng = np.random.default_rng(9)
    n = 6
    if kind == "int_into_float":
        series = [[(T0 + h * H + 60 * i, F, float(rng.integers(1, 1 << 20)) * 0.25) for h in range(2) for i in range(60)] for _ in range(n)]
        puts = [(s, T0 + H + 30 + 60 * j, L, int(rng.integers(-100, 30000))) for s in (0, 2, 3, 5) for j in range(0, 60, 7)]
    else:
        series = [[(T0 + h * H + 60 * i, L, int(rng.integers(-100, 30000))) for h in range(2) for i in range(60)] for _ in range(n)]
        puts = [(s, T0 + H + 30 + 60 * j, F, float(rng.integers(1, 1 << 20)) * 0.25) for s in (0, 2, 3, 5) for j in range(0, 60, 7)]
    a = store_batch(series, [s % 3 for s in range(n)])
    qs = [dsq(T0, T0 + 2 * H, "sum", "sum", 60000), dsq(T0, T0 + 2 * H, "max", "max", 60000)]
    with engine.options(**opts):
        info, _ = check_put(eng, a, puts, False, f"{kind} {opts}", queries=qs)
    assert (info.rows_added, info.rows_walked) == (0, 4)


@gpu
def test_single_datapoint_fixup(eng):
    """A resident one-datapoint row holding an 8-byte float under flags 0xB, plus one put."""
    q = struct.pack(">H", (100 << 4) | 0xB)
    a = synth.from_series([[(T0, q, b"\x00\x00\x00\x00" + struct.pack(">f", 1.5))], [sec_row(T0, [10], [3])]], [0, 1])
    info, exp = check_put(eng, a, [(0, T0 + 200, F, 2.5), (1, T0 + 200, L, 4)], False, "fixup", tail=0)
    assert bytes(exp.batch.val[:9]) == struct.pack(">f", 1.5) + struct.pack(">f", 2.5) + b"\x00" and info.rows_walked == 2
    assert check_put(eng, a, [(0, T0 + 100, F, 2.5)], False, "fixup, conflict")[0] == ID
    info, exp = check_put(eng, a, [(0, T0 + 100, F, 1.5)], False, "fixup, same bytes")
    assert bytes(exp.batch.val[:4]) == struct.pack(">f", 1.5) and exp.batch.row_val_off[1] == 4
    bad = synth.from_series([[(T0, q, b"\x00\x00\x00\x01" + struct.pack(">f", 1.5))]], [0])
    assert check_put(eng, bad, [(0, T0 + 200, F, 2.5)], False, "fixup, corrupted", queries=[])[0] == ID


# ---- 4. regular rows ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("step", [20, 7], ids=["continues", "breaks"])
def test_regular_rows(eng, step):
    rng = np.random.default_rng(13)
    series = [[(T0 + 10 + 20 * i, F, float(rng.integers(1, 1 << 20)) * 0.25) for i in range(100)] for _ in range(3)]
    a = store_batch(series, [0, 0, 1])
    eng.load(a)
    assert (eng.debug_regular()[0][:, 1] == 20).all()
    puts = [(s, T0 + 10 + 20 * 99 + step, F, 0.25 * (s + 1)) for s in range(3)]
    info, _ = check_put(eng, a, puts, False, f"regular step {step}", tail=3,
                        queries=[dsq(T0, T0 + H, "max", "max", 60000), abi.new_query(T0, T0 + H - 1, "max")])
    eng.load(a)
    eng.put(puts)
    assert (eng.debug_regular()[0][:, 1] == (20 if step == 20 else 0)).all()


# ---- 5. flags ----------------------------------------------------------------------------------------
def flagged(eng):
    return [bool(f & UNSORTED) for f in eng.debug_rows()[1]]


@gpu
def test_flags(eng):
    past = [sec_row(T0, [0, 3700], [1, 2]), sec_row(T0 + H, [50, 200], [3, 4])]   # the second row starts before the first ends
    a = synth.from_series([past, [sec_row(T0, [0, 3700], [1, 2])]], [0, 1])
    qs = [dsq(T0, T0 + 2 * H, "sum", "sum", 60000)]
    eng.load(a)
    assert flagged(eng) == [False, True, False]
    # the cause rewritten: the flagged row behind it is a suspect, indexed again, and stays flagged
    info, _ = check_put(eng, a, [(0, T0 + 5, L, 9)], False, "cause rewritten", queries=qs, tail=0)
    assert info.rows_reindexed == 1
    # a row whose ROW_UNSORTED is owed to the row before it: the walk finds its own offsets increasing
    info, _ = check_put(eng, a, [(0, T0 + H + 300, L, 9)], False, "flag owed to the row before", queries=qs, tail=0)
    assert info.rows_walked == 1
    # a put that opens the hour after a row reaching past it: the new row is flagged as a fresh load flags it
    info, exp = check_put(eng, a, [(1, T0 + H + 10, L, 9)], False, "new row behind a long one", queries=qs)
    assert info.rows_added == 1
    eng.load(exp.batch)
    assert flagged(eng) == [False, True, False, True]


@gpu
def test_unsorted_cell_and_malformed_cell_are_refused(eng):
    from opentsdb_amd import engine
    bad = (T0 + H, struct.pack(">H", (10 << 4) | 7) + struct.pack(">H", (20 << 4) | 7), b"\x01\x02\x00")   # 8-byte values claimed
    a = synth.from_series([[sec_row(T0, [0, 900], [5, 6]), sec_row(T0 + H, [100, 40, 900], [14, 15, 16])],
                           [sec_row(T0, [0, 900], [5, 6]), bad]], [0, 1])
    q = dsq(T0, T0 + H, "sum", "sum", 60000)                 # (the malformed row's hour throws when read)
    for walk in (-1, 1):
        with engine.options(PUT_WALK=walk):
            eng.load(a)
            before = eng.run(q), eng.debug_rows(), eng.download(), sizes(eng), eng.debug_regular()[0]
            assert put_code(eng, [(0, T0 + H + 500, L, 1)], False) == NI
            assert "do not strictly increase" in engine.lib().tsdbhip_last_error().decode()
            assert put_code(eng, [(0, T0 + 5, L, 1), (1, T0 + H + 500, L, 1)], True) == ID
            assert "malformed" in engine.lib().tsdbhip_last_error().decode()
            after = eng.run(q), eng.debug_rows(), eng.download(), sizes(eng), eng.debug_regular()[0]
            identical(before[0], after[0], "refused")
            for x, y in zip(before[1], after[1]):
                np.testing.assert_array_equal(x, y)
            batches_equal(before[2], after[2])
            assert before[3] == after[3]
            np.testing.assert_array_equal(before[4], after[4])
            # and the rows beside them still take puts
            assert eng.put([(0, T0 + 1000, L, 7), (1, T0 + 1000, L, 7)]).rows_tail == (0 if walk == 1 else 2)


@gpu
def test_illegal_arguments_leave_the_batch(eng):
    from opentsdb_amd import engine
    a = store_batch([FIVE, FIVE], [0, 1])
    qs = std_queries(T0, T0 + H)
    eng.load(a)
    before = state(eng, qs)
    lib = engine.lib()

    def code(points, flags=0, n=None):
        pts = points if isinstance(points, np.ndarray) else abi.make_points(points)
        return lib.tsdbhip_put(eng.ctx, pts.ctypes.data if len(pts) else None, len(pts) if n is None else n, flags, None)

    ok = (0, T0 + 50, L, 1)
    assert code([], n=1) == IA and code([ok], n=-1) == IA and code([ok], flags=2) == IA
    assert code([ok, (2, T0 + 50, L, 1)]) == IA and code([(-1, T0 + 50, L, 1)]) == IA
    for field, value in (("kind", 0), ("kind", 4), ("reserved", 1), ("timestamp", -1), ("timestamp", 10_000_000_000_000),
                         ("timestamp", ((1 << 32) + 3600) * 1000)):
        pts = abi.make_points([ok, ok])
        pts[field][1] = value
        assert code(pts) == IA, (field, value)
    for kind, bits in ((F, 0x7FC00000), (F, 0x7F800000), (F, 0xFF800000), (D, 0x7FF8 << 48), (D, 0x7FF0 << 48), (D, 0xFFF0 << 48)):
        pts = abi.make_points([ok, (1, T0 + 50, kind, 0.0)])
        pts["bits"][1] = bits
        assert code(pts) == IA, (kind, hex(bits))
    assert "NaN or Infinite" in lib.tsdbhip_last_error().decode()
    same_state(state(eng, qs), before, qs, "refused arguments")
    assert code([]) == 0                                       # n == 0: a no-op
    same_state(state(eng, qs), before, qs, "no points")
    assert code([(0, 9_999_999_999_999, L, 1)]) == IA          # the last legal ms timestamp: its base is above 2^32
    assert "2^32" in lib.tsdbhip_last_error().decode()
    same_state(state(eng, qs), before, qs, "base above 2^32")
    assert code([ok]) == 0


@gpu
def test_not_implemented_contexts(eng):
    from opentsdb_amd import engine
    from opentsdb_amd.rollup_read import make_rollup_batch
    a = store_batch([FIVE, FIVE], [0, 1])
    ok = [(0, T0 + 50, L, 1)]
    iv = engine.rollup_interval("10m", "1d")
    cell = (struct.pack(">H", (0 << 4) | 0x7), struct.pack(">q", 5))
    eng.load_rollup(make_rollup_batch([(None, [(T0, [cell], [])])], [0], iv, False))
    assert put_code(eng, ok, False) == NI
    eng.load_shard(a, engine.SHARD_SPANS, 0, a.n_series)
    q = dsq(T0, T0 + H, "sum", "sum", 60000)
    before = eng.run(q)
    assert put_code(eng, ok, False) == NI
    identical(before, eng.run(q), "shard batch untouched")
    md = engine.Engine(devices=[0, 0])
    try:
        md.load(a)
        assert put_code(md, ok, False) == NI
    finally:
        md.close()


@gpu
def test_row_that_failed_its_compaction_at_load_cells(eng):
    """A row that throws at tsdbhip_load_cells is not resident; only the compaction-error list makes a
    read of its hour throw.  The store still holds the bad cells, so a put into that hour is refused
    (a row from the puts alone would answer what the reference refuses), the batch stays as it was,
    the query still throws, and puts elsewhere keep the error."""
    from opentsdb_amd import engine
    from opentsdb_amd.engine import EngineError
    from tests.append_util import int_points
    rng = np.random.default_rng(11)
    good = [int_points(rng, T0 + np.arange(0, 2 * H, 60), 0, 1000) for _ in range(3)]
    q1, q2 = struct.pack(">H", (10 << 4) | 0), struct.pack(">H", (20 << 4) | 0)
    cells = lambda rows: [(b, [(q, v, None)]) for b, q, v in rows]   # noqa: E731
    bad_row = (T0 + H, [(q1, b"\x01", None), (q1 + q2, b"\x02\x03\x00", None)])   # a second twice, with another value
    series = [cells(good[0].rows(None, T0 + H)), cells(good[1].rows(None, T0 + H)) + [bad_row], cells(good[2].rows())]
    q = dsq(T0, T0 + 2 * H, "sum", "sum", 600000)
    first_hour = dsq(T0, T0 + H, "sum", "sum", 600000)
    for walk in (-1, 1):
        with engine.options(PUT_WALK=walk):
            eng.load_cells(abi.HostCellBatch.from_rows(series, [0, 0, 1]))
            with pytest.raises(EngineError) as e0:
                eng.run(q)
            assert e0.value.java == "IllegalDataException"
            before = eng.run(first_hour), eng.debug_rows(), eng.download(), sizes(eng)
            for fix in (False, True):
                assert put_code(eng, [(0, T0 + H + 5, L, 1), (1, T0 + H + 500, L, 7)], fix) == ID
                assert "failed its compaction" in engine.lib().tsdbhip_last_error().decode()
            after = eng.run(first_hour), eng.debug_rows(), eng.download(), sizes(eng)
            identical(before[0], after[0], "refused")
            for x, y in zip(before[1], after[1]):
                np.testing.assert_array_equal(x, y)
            batches_equal(before[2], after[2])
            assert before[3] == after[3]
            with pytest.raises(EngineError) as e1:
                eng.run(q)
            assert (e1.value.code, str(e1.value)) == (e0.value.code, str(e0.value))
            # puts into other rows, the bad series' first hour among them, keep the error
            info = eng.put([(1, T0 + 30, L, 3), (0, T0 + H + 5, L, 1)])
            assert (info.rows_added, info.rows_walked) == (1, 1)
            with pytest.raises(EngineError) as e2:
                eng.run(q)
            assert (e2.value.code, str(e2.value)) == (e0.value.code, str(e0.value))


# ---- 6. sequences --------------------------------------------------------------------------------------
def hour_store(n=8, hours=3, seed=21):
    rng = np.random.default_rng(seed)
    # (two-byte integers: rows of one value length, which the tail route asks for)
    series = [[(T0 + h * H + 60 * i, L, int(rng.integers(200, 30000))) for h in range(hours) for i in range(50)] for _ in range(n)]
    return series, [s % 3 for s in range(n)]


def compare_with_fresh(eng, m, qs, ctx):
    got = state(eng, qs), eng.debug_regular()[0]
    rb, _ = restricted(m, m.group_id)
    for i, (q, g) in enumerate(zip(qs, got[0][0])):
        assert_groups_match(g, want_of(rb, q), agg_name(q), tol=0.0, ctx=f"{ctx} q{i} vs oracle")
    eng.load(rb)
    same_state(got[0], state(eng, qs), qs, ctx)
    np.testing.assert_array_equal(got[1], eng.debug_regular()[0])


@gpu
def test_put_put_regroup_put(eng):
    series, gids = hour_store()
    a = store_batch(series, gids)
    qs = std_queries(T0, T0 + 3 * H)
    p1 = [(s, T0 + 2 * H + 3000 + 60 * j, L, 1000 + 10 * s + j) for s in range(8) for j in range(2)]
    p2 = [(s, T0 + 2 * H + 3120 + 60 * j, L, 2000 + 10 * s + j) for s in range(8) for j in range(2)]
    eng.load(a)
    i1 = eng.put(p1)
    i2 = eng.put(p2)
    assert (i1.rows_tail, i2.rows_tail, i2.grew) == (8, 8, 0) and i2.qual_dead > i1.qual_dead > 0
    m = put_batch(put_batch(a, p1).batch, p2).batch
    ids = [1, EXCL, 0, 0, abi.GROUP_NONE, 1, EXCL, 2]
    eng.regroup(ids)
    p3 = [(s, T0 + H + 30 + 60 * j, L, -s - j) for s in (1, 4, 7) for j in range(3)]   # into a closed hour; series 1 is excluded
    i3 = eng.put(p3)
    assert (i3.rows_tail, i3.rows_walked) == (0, 3)
    m = put_batch(with_ids(m, ids), p3).batch
    compare_with_fresh(eng, m, qs, "put / put / regroup / put")


@gpu
def test_put_then_trim_reclaims_the_dead_bytes(eng):
    series, gids = hour_store()
    a = store_batch(series, gids)
    qs = std_queries(T0, T0 + 3 * H)
    puts = [(s, T0 + H + 30 + 60 * j, L, s + j) for s in range(8) for j in range(4)]
    eng.load(a)
    info = eng.put(puts)
    assert info.qual_dead > 0 and info.val_dead > 0
    t = eng.trim(T0, 0)
    assert t.packed == 1 and (t.qual_dead, t.val_dead) == (0, 0) and t.qual_reclaimed > 0 and t.val_reclaimed > 0
    compare_with_fresh(eng, put_batch(a, puts).batch, qs, "put / trim with pack")


@gpu
def test_put_then_last_returns_the_new_point(eng):
    series, gids = hour_store()
    a = store_batch(series, gids)
    eng.load(a)
    ts, bits, kind, _ = eng.last([2, 5], anchor_s=T0 + 3 * H - 1, back_scan=0)
    assert ts.tolist() == [(T0 + 2 * H + 60 * 49) * 1000] * 2
    eng.put([(2, T0 + 2 * H + 3500, L, -77), (5, (T0 + 2 * H + 3599) * 1000 + 999, D, 0.25), (5, T0 + 2 * H + 3599, L, 1)])
    ts, bits, kind, _ = eng.last([2, 5], anchor_s=T0 + 3 * H - 1, back_scan=0)
    assert ts.tolist() == [(T0 + 2 * H + 3500) * 1000, (T0 + 2 * H + 3599) * 1000 + 999]
    assert bits.astype(np.int64)[0] == -77 and bits[1:].view(np.float64)[0] == 0.25
    assert kind.tolist() == [abi.LAST_INT, abi.LAST_FLOAT]


@gpu
def test_rollup_and_preagg_cells_are_dropped(eng):
    from opentsdb_amd import engine
    rng = np.random.default_rng(31)
    pts = [quarter_points(rng, T0 + np.arange(0, 3 * H, 300)) for _ in range(4)]
    a = synth.from_series([p.rows() for p in pts], [0, 0, 1, 1])
    iv = engine.rollup_interval("10m", "1d")
    end = T0 + 3 * H
    eng.load(a)
    old = eng.rollup(iv, T0, end, FUNCS)
    assert len(old) and eng.preagg_run(iv, T0, end, "sum", FUNCS)[0]
    puts = [(s, T0 + 2 * H + 3400, F, 0.5) for s in range(4)]
    eng.put(puts)
    assert resident_cells(eng) == 0
    cells = eng.rollup(iv, T0, end, FUNCS)
    eng.load(put_batch(a, puts).batch)
    fresh = eng.rollup(iv, T0, end, FUNCS)
    for name in ("series", "base_time", "qualifier", "val_off", "value"):
        np.testing.assert_array_equal(getattr(cells, name), getattr(fresh, name), err_msg=name)


# ---- 7. one tick ---------------------------------------------------------------------------------------
@gpu
def test_one_tick(eng):
    """4096 series x 2 hour rows, one tail point a series: the live-ingest shape."""
    from opentsdb_amd import engine
    rng = np.random.default_rng(43)
    n = 4096
    ts = np.concatenate([T0 + np.arange(0, H, 60), T0 + H + np.arange(0, 1800, 60)])
    a = synth.from_series([quarter_points(rng, ts).rows() for _ in range(n)], [s % 8 for s in range(n)])
    puts = [(int(s), T0 + H + 1800, F, 0.25 * (s % 64 + 1)) for s in rng.permutation(n)]
    m = put_batch(a, puts).batch
    q = dsq(T0, T0 + 2 * H, "sum", "sum", 60000)
    want = O.run_query(m, q)
    eng.load(m)
    fresh = state(eng, [q]), eng.debug_regular()[0]
    for walk in (-1, 1):
        with engine.options(PUT_WALK=walk):
            eng.load(a)
            eng.run(q)
            info = eng.put(puts)
            got = state(eng, [q]), eng.debug_regular()[0]
        assert (info.rows_added, info.rows_tail, info.rows_walked) == ((0, n, 0) if walk < 0 else (0, 0, n))
        assert_groups_match(got[0][0][0], want, "sum", tol=0.0, ctx=f"tick walk={walk}")
        same_state(got[0], fresh[0], [q], f"tick walk={walk}")
        np.testing.assert_array_equal(got[1], fresh[1])


# ---- 8. ResidentSpans end to end -----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fix", [False, True], ids=["nofix", "fix"])
def test_resident_spans_put_equals_a_fresh_resident(eng, fix):
    from opentsdb_amd.query import ResidentSpans
    from tests.test_regroup_cpu import END, METRIC, QUERIES, START, TAGS, make_store, query
    st = make_store()
    st.fix_duplicates = fix
    rs = ResidentSpans(st, METRIC, START, END, engine=eng)
    rs.run(query(st, {"host": "*"}))                          # the old state
    key0 = (st._series_uids(METRIC, TAGS[0]))
    first = min(b for (m, t, b) in st.rows if (m, t) == key0)
    q0 = next(iter(st.rows[(key0[0], key0[1], first)].cells))
    t_dup = first + store_offset(q0)
    pts = [(TAGS[0], START + 3600 + 1, L, 5), (TAGS[1], (START + 2 * 3600 + 7) * 1000 + 250, D, 0.5), (TAGS[3], END - 1, F, 1.25)]
    info, ups = rs.put(pts)
    assert info.rows_tail + info.rows_walked == 3 and ups == []
    # a series the resident scan has not met: its hour is rescanned
    info, ups = rs.put([({"host": "new01", "dc": "lga"}, START + 30, L, 1), (TAGS[2], START + 31, L, 2)])
    assert info.rows_walked + info.rows_tail == 1 and len(ups) == 1 and ups[0].series_added == 1
    # a point onto a datapoint the resident cell holds, under the same qualifier with another value: the store
    # overwrites that cell version.  With fix_duplicates the engine keeps the put as well; without it the engine
    # refuses (the documented deviation) and the fallback rescans the hour, which the store reads without an error
    assert len(q0) == 2
    fl = q0[1] & 0xF
    old = st.rows[(key0[0], key0[1], first)].cells[q0]
    kind, val = (F, 123.0) if fl == 0xB else (D, 123.0) if fl == 0xF else (L, {0: 5, 1: 300, 3: 70000, 7: 1 << 40}[fl])
    if put_util_encode(t_dup, kind, val)[2] == old:
        val += 1
    assert put_util_encode(t_dup, kind, val)[1] == q0
    info, ups = rs.put([(TAGS[0], t_dup, kind, val)])
    if fix:
        assert info is not None and info.rows_walked == 1 and ups == []
        info, ups = rs.put([(TAGS[0], t_dup, D, 321.0)])      # another qualifier at that offset: the newest column wins
        assert info is not None and ups == []
    else:
        assert info is None and len(ups) == 1 and ups[0].rows_replaced >= 1
    got = {i: rs.run(query(st, tags)) for i, tags in enumerate(QUERIES)}
    spans = rs.spans
    fresh = ResidentSpans(st, METRIC, START, END, engine=eng)
    assert spans == fresh.spans and rs.span_keys == fresh.span_keys
    for i, tags in enumerate(QUERIES):
        exp = fresh.run(query(st, tags))
        assert len(got[i]) == len(exp), tags
        by = {d.group_key: d for d in got[i]}
        for d in exp:
            for name in ("ts", "bits", "is_int"):
                np.testing.assert_array_equal(getattr(by[d.group_key], name), getattr(d, name), err_msg=f"{tags} {name}")


def store_offset(q):
    from opentsdb_amd.store import qualifier_offset_ms
    return qualifier_offset_ms(q) // 1000
