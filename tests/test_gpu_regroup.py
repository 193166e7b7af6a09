"""GPU parity of tsdbhip_regroup (k_regroup.hip): new group ids and tag-filter verdicts for the
resident batch without a reload.

The expectation never comes from the engine: after regroup(ids) the context must answer as if
the loaded batch, restricted to the series with ids != GROUP_EXCLUDED and carrying the new ids,
had been loaded afresh -- so the expectation is the oracle over that restricted host batch
(restricted(), built with dist.select_series).  Every case first queries the OLD grouping over
the same time range (stale caches would show), regroups, compares with the oracle bit for bit,
and then compares array for array with the same engine after a fresh load of the restricted
batch.

Inputs are order-free -- integers, or multiples of 0.25 below 2^20 (tests/test_gpu_preagg.py's
stores: sums, two-point averages and the LERP fractions of their gaps are exact) -- so the default
unordered path must equal the oracle to the bit; test_inputs_are_order_free checks the claim on
the CPU for every query used on a float store.  Full-mantissa float64 values and `dev` run under
TSDB_QF_ORDERED, which is bit-exact by contract.  The rate query uses the max aggregator: a rate
is a quotient, not order-free under a sum.

The 3600-datapoint walker class is exercised at tile size 1 only: an oracle pass over enough
such series for T > 1 (8192 tiles) would take tens of seconds.
"""
from __future__ import annotations

import struct

import numpy as np
import pytest

from opentsdb_amd import abi, dist, synth
from oracle import oracle as O
from oracle import rollup as R
from tests.test_gpu_parity import assert_groups_match
from tests.test_gpu_preagg import (FUNCS, MIX_END, MIX_START, expected_cells, mixed_store, quarter_series,
                                    resident_cells)

gpu = pytest.mark.gpu

T0 = 1356998400
EXCL = abi.GROUP_EXCLUDED


@pytest.fixture(scope="module")
def eng():
    from opentsdb_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


# ---- the expectation's input ------------------------------------------------------------------
def with_ids(batch, ids):
    return abi.HostBatch(batch.series_row_ptr, batch.row_base_time, batch.row_qual_off, batch.row_val_off, batch.qual,
                         batch.val, np.asarray(ids, np.int32))


def restricted(batch, ids):
    """(the batch restricted to the series whose id is not GROUP_EXCLUDED, batch order kept, with
    the new ids; the kept batch positions)."""
    ids = np.asarray(ids, np.int32)
    kept = np.flatnonzero(ids != EXCL)
    return with_ids(dist.select_series(batch, kept), ids[kept]), kept


def resident_order(gid):
    """Group ids in resident order: groups ascending, then the ungrouped series (-1)."""
    g = np.asarray(gid, np.int32)
    return np.concatenate([np.sort(g[g >= 0]), g[g < 0]])


def dsq(start, end, agg, fn, interval_ms, **kw):
    return abi.new_query(start, end - 1, agg, ds_function=abi.AGG[fn], ds_interval_ms=interval_ms, **kw)


def want_of(rb, q):
    return O.run_query(rb, q) if rb.n_series else []


def identical(a, b, ctx):
    assert len(a) == len(b), (ctx, len(a), len(b))
    for (g1, t1, b1, i1), (g2, t2, b2, i2) in zip(a, b):
        assert g1 == g2, (ctx, g1, g2)
        for name, x, y in (("ts_ms", t1, t2), ("value_bits", b1, b2), ("is_int", i1, i2)):
            np.testing.assert_array_equal(x, y, err_msg=f"{ctx} g{g1}: {name}")


def agg_name(q):
    return abi.AGGREGATOR_NAMES[q.aggregator]


def check_regroup(eng, batch, ids, queries, ctx, loaded=False):
    """One case: load (unless the caller has), query the old grouping, regroup, oracle, fresh load."""
    if not loaded:
        eng.load(batch)
    for q in queries:
        eng.run(q)                                   # the old grouping, same time range
    eng.regroup(ids)
    rb, kept = restricted(batch, ids)
    assert eng.n_series() == len(kept)
    got = [eng.run(q) for q in queries]
    for i, (q, g) in enumerate(zip(queries, got)):
        assert_groups_match(g, want_of(rb, q), agg_name(q), tol=0.0, ctx=f"{ctx} q{i} vs oracle")
    np.testing.assert_array_equal(eng.resident_groups(), resident_order(rb.group_id))
    eng.load(rb)
    for i, (q, g) in enumerate(zip(queries, got)):
        identical(g, eng.run(q), f"{ctx} q{i} vs fresh load")
    return got, rb, kept


def scatter_ids(n, n_groups, excl_every=5, ungrouped=(1,)):
    """Ids unrelated to the batch order: a multiplicative hash of the position; every
    excl_every-th series filtered out, a few ungrouped."""
    i = np.arange(n, dtype=np.int64)
    ids = ((i * 2654435761 >> 5) % n_groups).astype(np.int32)
    if excl_every:
        ids[excl_every - 1::excl_every] = EXCL
    for u in ungrouped:
        if u < n:
            ids[u] = abi.GROUP_NONE
    return ids


# ---- row classes at tile size 1 -----------------------------------------------------------------
def int_series(rng, ts_s, lo, hi, ms=False):
    ts = np.asarray(ts_s, np.int64) * 1000
    n = len(ts)
    return synth.encode_rows(ts, rng.integers(lo, hi, n), None, np.zeros(n, int), np.full(n, ms))


def mixed_kind_series(rng, ts_s, s):
    """Integer, float32 and float64 values in one row; millisecond qualifiers on every other series."""
    ts = np.asarray(ts_s, np.int64) * 1000 + (250 if s % 2 else 0)
    n = len(ts)
    kind = rng.integers(0, 3, n)
    fv = rng.integers(1, 1 << 22, n).astype(np.float64) * 0.25
    fv[kind == 2] += float(2 ** 25)
    return synth.encode_rows(ts, rng.integers(-5000, 5000, n), fv, kind, np.full(n, bool(s % 2)))


def class_store(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "short_f32":      # one row of 360 float32 points a series: k_short
        rows = [quarter_series(rng, T0 + np.arange(0, 3600, 10)) for _ in range(12)]
        end = T0 + 3600
    elif name == "short_int":    # one row of 1-2-byte integers: k_short over val2
        rows = [int_series(rng, T0 + np.arange(0, 3600, 10), -100, 30000) for _ in range(12)]
        end = T0 + 3600
    elif name == "rows":         # three hour rows of 120 points: k_rows
        rows = [quarter_series(rng, T0 + np.arange(0, 3 * 3600, 30)) for _ in range(10)]
        end = T0 + 3 * 3600
    elif name == "walker":       # a 3600-point row: k_fast's walker
        rows = [quarter_series(rng, T0 + np.arange(0, 3600, 1)) for _ in range(9)]
        end = T0 + 3600
    elif name == "mixed":        # integer / float / millisecond rows: k_grid
        rows = [mixed_kind_series(rng, T0 + np.arange(0, 7200, 20), s) for s in range(12)]
        end = T0 + 7200
    elif name == "hwin":         # a day of 1m buckets over hour rows: k_hwin, K = 1440
        rows = [quarter_series(rng, T0 + np.arange(0, 86400, 30)) for _ in range(9)]
        end = T0 + 86400
    else:
        raise KeyError(name)
    n = len(rows)
    return synth.from_series(rows, [i % 3 for i in range(n)]), end


CLASSES = ["short_f32", "short_int", "rows", "walker", "mixed", "hwin"]


@gpu
@pytest.mark.parametrize("name", CLASSES)
def test_row_classes(eng, name):
    batch, end = class_store(name)
    queries = [dsq(T0, end, "sum", "sum", 60000), dsq(T0, end, "max", "max", 60000)]
    ids = scatter_ids(batch.n_series, 4)
    got, rb, _ = check_regroup(eng, batch, ids, queries, name)
    assert len(got[0]) == len(set(rb.group_id[rb.group_id >= 0].tolist())) >= 3


@gpu
def test_ordered_full_mantissa(eng):
    """Full 53-bit mantissa float64 under TSDB_QF_ORDERED (k_seq_* / k_ordered)."""
    batch = synth.generate(12, T0, 600, 10000, value_kind=4, n_groups=2)
    queries = [dsq(T0, T0 + 6000, "sum", "sum", 60000, flags=abi.QF_ORDERED),
               dsq(T0, T0 + 6000, "avg", "avg", 600000, flags=abi.QF_ORDERED)]
    check_regroup(eng, batch, scatter_ids(12, 3), queries, "ordered f64")


# ---- query kinds over the mixed store -------------------------------------------------------
MIX_IDS = [1, EXCL, 0, 0, 1, 2, abi.GROUP_NONE, 2, 3]   # was [0, 0, 0, 1, 1, -1, 2, 2, 3]


def mix_queries():
    ten = 600000
    return {
        "sum": dsq(MIX_START, MIX_END, "sum", "avg", ten),
        "max": dsq(MIX_START, MIX_END, "max", "avg", ten),
        "dev": dsq(MIX_START, MIX_END, "dev", "avg", ten, flags=abi.QF_ORDERED),
        "p99": dsq(MIX_START, MIX_END, "p99", "avg", ten),
        "none": dsq(MIX_START, MIX_END, "none", "avg", ten),
        "raw": abi.new_query(MIX_START, MIX_END - 1, "sum"),
        "rate": dsq(MIX_START, MIX_END, "max", "avg", ten, rate=True),
    }


def reversed_in_groups(batch):
    """The same series in reverse batch order: every group's SpanGroup order reversed."""
    order = np.arange(batch.n_series)[::-1]
    return with_ids(dist.select_series(batch, order), batch.group_id[order])


def test_inputs_are_order_free():
    """The oracle over the restricted mixed store and over the same series in reverse order gives
    the same bits for every unordered group-by query the GPU tests run on a float store."""
    rb, _ = restricted(mixed_store(), MIX_IDS)
    rev = reversed_in_groups(rb)
    qs = mix_queries()
    multi = [dsq(MIX_START, MIX_END, a, "avg", 600000) for a in ("avg", "min", "max", "count")]
    for name, q in [(k, qs[k]) for k in ("sum", "max", "p99", "raw", "rate")] + [("multi", q) for q in multi]:
        ra, rv = O.run_query(rb, q), O.run_query(rev, q)
        assert len(ra) == len(rv) == 3, name
        identical(ra, rv, name)
    for name in ("short_f32", "rows", "walker", "mixed", "hwin"):
        batch, end = class_store(name)
        rb, _ = restricted(batch, scatter_ids(batch.n_series, 4))
        for q in (dsq(T0, end, "sum", "sum", 60000), dsq(T0, end, "max", "max", 60000)):
            identical(O.run_query(rb, q), O.run_query(reversed_in_groups(rb), q), name)


@gpu
def test_query_kinds(eng):
    qs = mix_queries()
    got, rb, kept = check_regroup(eng, mixed_store(), MIX_IDS, list(qs.values()), "mixed store")
    by = dict(zip(qs, got))
    assert [g for g, *_ in by["sum"]] == [0, 1, 2]          # group 3 lies outside the range
    assert len(by["none"]) == 7 and [g for g, *_ in by["none"]] == list(range(7))   # ranks over live spans
    assert len(by["raw"]) == 3 and len(by["rate"]) == 3


@gpu
def test_run_multi(eng):
    batch = mixed_store()
    qs = [dsq(MIX_START, MIX_END, a, "avg", 600000) for a in ("avg", "min", "max", "count")]
    eng.load(batch)
    eng.run_multi(qs)
    eng.regroup(MIX_IDS)
    rb, _ = restricted(batch, MIX_IDS)
    got = eng.run_multi(qs)
    for q, g in zip(qs, got):
        assert_groups_match(g, O.run_query(rb, q), agg_name(q), tol=0.0, ctx=f"multi {agg_name(q)}")
    eng.load(rb)
    for q, g, f in zip(qs, got, eng.run_multi(qs)):
        identical(g, f, f"multi {agg_name(q)} vs fresh load")


@gpu
def test_per_span_calendar(eng):
    """2dc is anchored on each span's first datapoint; the regroup filters out the earliest span,
    so the first visible span -- and the cached calendar plan -- change."""
    from opentsdb_amd.engine import parse_downsample
    rng = np.random.default_rng(5)
    rows = [int_series(rng, T0 + d * 86400 + np.arange(0, (9 - d) * 86400, 6 * 3600), 0, 1000) for d in (0, 1, 1, 2, 3, 0)]
    batch = synth.from_series(rows, [0, 0, 1, 1, 2, 2])
    q = abi.new_query(T0, T0 + 9 * 86400 - 1, "sum")
    p = parse_downsample("2dc-sum")
    for f in ("ds_function", "ds_fill", "ds_all", "ds_calendar", "ds_interval_ms"):
        setattr(q, f, getattr(p, f))
    check_regroup(eng, batch, [EXCL, 1, 1, 0, 0, EXCL], [q], "2dc")


@gpu
def test_rollup_and_preagg_cells(eng):
    from opentsdb_amd import engine
    batch = mixed_store()
    iv = engine.rollup_interval("10m", "1d")
    eng.load(batch)
    old = eng.rollup(iv, MIX_START, MIX_END, FUNCS)
    n_old = eng.preagg_run(iv, MIX_START, MIX_END, "sum", FUNCS)[0]
    assert len(old) and n_old
    eng.regroup(MIX_IDS)
    # the old grouping's cells are gone: a download writes nothing but the end offset
    ser = np.full(len(old), -7, np.int32)
    voff = np.full(len(old) + 1, 2 ** 63, np.uint64)
    assert engine.lib().tsdbhip_rollup_download(eng.ctx, ser.ctypes.data, None, None, voff.ctypes.data, None) == 0
    assert voff[0] == 0 and (ser == -7).all()
    assert resident_cells(eng) == 0
    rb, kept = restricted(batch, MIX_IDS)
    cells = eng.rollup(iv, MIX_START, MIX_END, FUNCS)
    exp = R.generate(rb, R.Interval("10m", "1d"), MIX_START, MIX_END, FUNCS)
    got = [cells.cell(i) for i in range(len(cells))]
    assert len(got) == len(exp) > 0
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g == (int(kept[e[0]]),) + tuple(e[1:]), (i, g, e)   # series: positions of the batch as loaded
    pre = eng.preagg(iv, MIX_START, MIX_END, "sum", FUNCS)
    pexp = expected_cells(rb, R.Interval("10m", "1d"), MIX_START, MIX_END, "sum", FUNCS)
    pgot = [pre.cell(i) for i in range(len(pre))]
    assert pgot == pexp and len(pexp) > 0
    # and array for array against a fresh load
    eng.load(rb)
    fresh = eng.rollup(iv, MIX_START, MIX_END, FUNCS)
    np.testing.assert_array_equal(cells.series, kept[fresh.series])
    for name in ("base_time", "qualifier", "val_off", "value"):
        np.testing.assert_array_equal(getattr(cells, name), getattr(fresh, name), err_msg=name)
    fpre = eng.preagg(iv, MIX_START, MIX_END, "sum", FUNCS)
    for name in ("func_index", "group", "base_time", "qual_off", "qualifier", "val_off", "value"):
        np.testing.assert_array_equal(getattr(pre, name), getattr(fpre, name), err_msg=name)


# ---- real tiles ------------------------------------------------------------------------------
@gpu
def test_real_tiles(eng):
    """524 288 series is the smallest count at which build_tiles keeps T = 64 (it needs
    ceil(n / 64) >= 8192); 7 groups by a hash of the position scatter every tile's series over
    the blobs.  Then every fourth series filtered out: 393 216 visible, T = 32."""
    n = 524288
    eng.synth(n, T0, 12, 10000, 1, 4, 1000)
    host = eng.download()
    assert host.n_series == n
    queries = [dsq(T0, T0 + 120, "sum", "sum", 60000), dsq(T0, T0 + 120, "max", "max", 60000)]
    ids = scatter_ids(n, 7, excl_every=0, ungrouped=())
    for q in queries:
        eng.run(q)
    for step, excl in (("T=64", 0), ("T=32", 4)):
        ids2 = ids.copy()
        if excl:
            ids2[excl - 1::excl] = EXCL
        eng.regroup(ids2)
        rb, kept = restricted(host, ids2)
        assert eng.n_series() == len(kept) == (n if not excl else n - n // 4)
        for i, q in enumerate(queries):
            got = eng.run(q)
            assert len(got) == 7
            assert_groups_match(got, O.run_query(rb, q, threads=8), agg_name(q), tol=0.0, ctx=f"{step} q{i}")


# ---- sequences -------------------------------------------------------------------------------
@gpu
def test_sequences(eng):
    """A -> B (a third excluded) -> C (those back, others excluded, one group left empty) -> all
    excluded -> A: every step against the oracle, the last A bit-identical to the first."""
    batch = mixed_store()
    n = batch.n_series
    A = batch.group_id.copy()
    B = np.array([2, EXCL, 1, 0, EXCL, 0, 1, EXCL, 2], np.int32)
    Cc = np.array([EXCL, 3, EXCL, 0, 3, abi.GROUP_NONE, EXCL, 0, 1], np.int32)   # group 2 is empty
    qs = [dsq(MIX_START, MIX_END, "sum", "avg", 600000), dsq(MIX_START, MIX_END, "none", "avg", 600000),
          abi.new_query(MIX_START, MIX_END - 1, "sum")]
    eng.load(batch)
    first = None
    for name, ids in (("A", A), ("B", B), ("C", Cc), ("none", np.full(n, EXCL, np.int32)), ("A2", A)):
        eng.regroup(ids)
        rb, kept = restricted(batch, ids)
        assert eng.n_series() == len(kept)
        got = [eng.run(q) for q in qs]
        for i, (q, g) in enumerate(zip(qs, got)):
            assert_groups_match(g, want_of(rb, q), agg_name(q), tol=0.0, ctx=f"{name} q{i}")
        if name == "A":
            first = got
        if name == "none":
            assert all(g == [] for g in got)
    for i, (a, b) in enumerate(zip(first, got)):
        identical(a, b, f"A again q{i}")
    np.testing.assert_array_equal(eng.download().group_id, resident_order(A))


# ---- load_cells: a row whose compaction fails ---------------------------------------------------
@gpu
def test_load_cells_compaction_error_of_an_excluded_series(eng):
    from opentsdb_amd.engine import EngineError
    rng = np.random.default_rng(11)
    good = [int_series(rng, T0 + np.arange(0, 3600, 60), 0, 1000) for _ in range(3)]
    q1 = struct.pack(">H", (10 << 4) | 0)
    q2 = struct.pack(">H", (20 << 4) | 0)
    # the same second in a single-datapoint column and in a compacted column, with another value
    bad = [(T0, [(q1, b"\x01", None), (q1 + q2, b"\x02\x03\x00", None)])]
    series = [[(b, [(q, v, None)]) for b, q, v in good[0]], bad] + [[(b, [(q, v, None)]) for b, q, v in g] for g in good[1:]]
    eng.load_cells(abi.HostCellBatch.from_rows(series, [0, 0, 1, 1]))
    q = dsq(T0, T0 + 3600, "sum", "sum", 600000)
    with pytest.raises(EngineError) as e0:
        eng.run(q)
    assert e0.value.java == "IllegalDataException"
    eng.regroup([1, EXCL, 0, 1])
    want = O.run_query(synth.from_series(good, [1, 0, 1]), q)
    assert_groups_match(eng.run(q), want, "sum", tol=0.0, ctx="bad series excluded")
    eng.regroup([0, 1, 1, EXCL])
    with pytest.raises(EngineError) as e1:
        eng.run(q)
    assert (e1.value.code, str(e1.value)) == (e0.value.code, str(e0.value))


# ---- refusals --------------------------------------------------------------------------------
def regroup_code(e, ids, n=None):
    from opentsdb_amd import engine
    ids = np.ascontiguousarray(ids, np.int32)
    return engine.lib().tsdbhip_regroup(e.ctx, ids.ctypes.data, len(ids) if n is None else n)


@gpu
def test_illegal_arguments_leave_the_grouping(eng):
    from opentsdb_amd import engine
    batch = mixed_store()
    qs = [dsq(MIX_START, MIX_END, "sum", "avg", 600000), dsq(MIX_START, MIX_END, "none", "avg", 600000)]
    eng.load(batch)
    eng.regroup(MIX_IDS)
    before = [eng.run(q) for q in qs]
    assert regroup_code(eng, np.zeros(8, np.int32)) == abi.TSDB_E_ILLEGAL_ARGUMENT          # one series short
    assert regroup_code(eng, np.zeros(10, np.int32)) == abi.TSDB_E_ILLEGAL_ARGUMENT
    assert regroup_code(eng, [0, 0, 0, 0, -3, 0, 0, 0, 0]) == abi.TSDB_E_ILLEGAL_ARGUMENT
    assert engine.lib().tsdbhip_regroup(eng.ctx, None, 9) == abi.TSDB_E_ILLEGAL_ARGUMENT
    assert eng.n_series() == 8
    for i, (q, b) in enumerate(zip(qs, before)):
        identical(b, eng.run(q), f"after refused calls q{i}")


@gpu
def test_not_implemented(eng):
    from opentsdb_amd import engine
    from opentsdb_amd.rollup_read import make_rollup_batch
    iv = engine.rollup_interval("10m", "1d")
    cell = (struct.pack(">H", (0 << 4) | 0x7), struct.pack(">q", 5))
    eng.load_rollup(make_rollup_batch([(None, [(T0, [cell], [])])], [0], iv, False))
    assert regroup_code(eng, [0]) == abi.TSDB_E_NOT_IMPLEMENTED
    batch = mixed_store()
    eng.load_shard(batch, engine.SHARD_SPANS, 0, batch.n_series)
    assert regroup_code(eng, MIX_IDS) == abi.TSDB_E_NOT_IMPLEMENTED
    q = dsq(MIX_START, MIX_END, "sum", "avg", 600000)
    assert_groups_match(eng.run(q), O.run_query(batch, q), "sum", tol=0.0, ctx="shard batch untouched")
    eng.load(batch)
    assert regroup_code(eng, MIX_IDS) == 0   # and a whole load regroups
    md = engine.Engine(devices=[0, 0])
    try:
        md.load(batch)
        assert regroup_code(md, MIX_IDS) == abi.TSDB_E_NOT_IMPLEMENTED
    finally:
        md.close()


# ---- ResidentSpans end to end --------------------------------------------------------------------
@gpu
def test_resident_spans_equal_tsdb_query(eng):
    from opentsdb_amd.query import ResidentSpans
    from tests.test_regroup_cpu import END, METRIC, QUERIES, START, make_store, query
    store = make_store()
    windows = [(START, END - 1), (START + 2 * 3600, END - 1)]
    want = {}
    for w, (s, e) in enumerate(windows):
        for i, tags in enumerate(QUERIES):
            q = query(store, tags, start=s, end=e)
            q.runner = eng.run_batch
            want[w, i] = q.run()
    rs = ResidentSpans(store, METRIC, START, END, engine=eng)
    for w, (s, e) in enumerate(windows):
        for i, tags in enumerate(QUERIES):
            got = rs.run(query(store, tags, start=s, end=e))
            exp = want[w, i]
            assert len(got) == len(exp), (w, tags)
            assert len({d.group_key for d in exp}) == len(exp)
            by = {d.group_key: d for d in got}
            for d in exp:
                g = by[d.group_key]
                for name in ("ts", "bits", "is_int"):
                    np.testing.assert_array_equal(getattr(g, name), getattr(d, name), err_msg=f"{w} {tags} {name}")
    # nine host values over the eleven resident series, five of them once the first-hour series is out of
    # the scan range and web02 has one span left; the unknown tag value matches nothing
    assert len(want[0, 1]) == 9 and len(want[0, 3]) == 4 and want[0, 5] == [] and want[1, 5] == []
