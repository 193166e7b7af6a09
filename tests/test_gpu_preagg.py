"""GPU parity of pre-aggregate generation (tsdbhip_preagg_run, k_preagg.hip): the group-by
cells of a rollup interval's group-by table (form A) and of the default interval's (form B).

The expectation never comes from the engine.  The cells of function i are defined as the
DataPoints of the query (start_s, end_s - 1, group-by aggregator, func[i], fill none, the
interval), so the expectation is oracle.run_query for that query, encoded here with
oracle.rollup.basetime / qualifier / encode_value(v, False) (form A) or the hour row and
Internal.buildQualifier of a second timestamp (form B).  Every cell is compared byte for byte:
function index, group, base time, qualifier, value.

Inputs are multiples of 0.25 in [0.25, 2^20) (plus a few values at 2^25 + 0.25, which need a
float64 cell): every sum, and every LERP value across a gap of one or three missing buckets
(fractions 1/2, 1/4, 3/4), is exact in a double in any order, so the default (unordered) path
must equal the oracle bit for bit -- test_inputs_are_order_free checks that claim on the CPU.
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import pytest

from opentsdb_amd import abi, synth
from oracle import oracle as O
from oracle import rollup as R

gpu = pytest.mark.gpu

T0 = 1356998400   # 2013-01-01 00:00 UTC
FUNCS = (("sum", 0), ("count", 1), ("max", 2), ("min", 3))
BIG = float(2 ** 25) + 0.25   # not a float32: a float64 cell


@pytest.fixture(scope="module")
def eng():
    from opentsdb_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


# ---- inputs ---------------------------------------------------------------------------------
def quarter_series(rng, ts_s, big_at=()):
    """One series' rows: float values that are multiples of 0.25 in [0.25, 2^20) at ts_s
    (seconds), 2^25 + 0.25 at the indices big_at."""
    ts_s = np.asarray(ts_s, np.int64)
    fv = rng.integers(1, 1 << 22, len(ts_s)).astype(np.float64) * 0.25
    for i in big_at:
        fv[i] = BIG
    kind = np.where(fv.astype(np.float32).astype(np.float64) == fv, 1, 2)
    return synth.encode_rows(ts_s * 1000, None, fv, kind, np.zeros(len(ts_s), bool))


def drop_slots(ts_s, start, interval, slots):
    """ts_s without the points of the given slots of the grid (start, interval)."""
    ts_s = np.asarray(ts_s, np.int64)
    k = (ts_s - start) // interval
    return ts_s[~np.isin(k, list(slots))]


MIX_START = T0 + 40 * 60
MIX_END = MIX_START + 68 * 600   # 11 h 20 m of 10m slots: 68, across a 64-slot boundary


def mixed_store(perm=None):
    """3 groups that emit, one ungrouped series, one group wholly outside [start, end), interior
    gaps of one and three buckets (LERP contributions), late starts and early ends (sparse emit
    flags).  Points every 5 minutes; group 0 starts before the range and runs past its end."""
    rng = np.random.default_rng(20130101)
    grid = lambda a, b: np.arange(MIX_START + a * 600, MIX_START + b * 600, 300)   # noqa: E731
    full = np.arange(T0, MIX_END + 3600, 300)
    series = [
        (0, quarter_series(rng, full, big_at=(30, 31, 77))),
        (0, quarter_series(rng, drop_slots(full, MIX_START, 600, {12}))),
        (0, quarter_series(rng, drop_slots(full, MIX_START, 600, {40, 41, 42, 63}), big_at=(5,))),
        (1, quarter_series(rng, grid(20, 68))),                 # late start
        (1, quarter_series(rng, grid(0, 51))),                  # early end
        (-1, quarter_series(rng, full)),                        # no group-by tag: takes no part
        (2, quarter_series(rng, grid(10, 41))),                 # slots 10..40 only
        (2, quarter_series(rng, drop_slots(grid(30, 61), MIX_START, 600, {50}))),
        (3, quarter_series(rng, np.arange(MIX_END + 3 * 3600, MIX_END + 5 * 3600, 300))),   # outside the range
    ]
    if perm is not None:   # the series of each group in another order (SpanGroup order changes)
        series = [series[i] for i in perm]
    return synth.from_series([s for _, s in series], [g for g, _ in series])


def regular_store(n_series, n_groups, start, step, n_points, seed):
    rng = np.random.default_rng(seed)
    ts = start + np.arange(n_points) * step
    rows = [quarter_series(rng, ts) for _ in range(n_series)]
    return synth.from_series(rows, [i * n_groups // n_series for i in range(n_series)])


# ---- the expectation: the oracle's DataPoints, encoded -------------------------------------
def query_of(start, end, gagg, fn, interval_ms, flags=0):
    return abi.new_query(start, end - 1, gagg, ds_function=abi.AGG[fn], ds_interval_ms=interval_ms, flags=flags)


def expected_cells(batch, iv, start, end, gagg, funcs, flags=0, ds_interval_ms=0):
    """iv: an oracle.rollup.Interval (form A) or None (form B)."""
    out = []
    interval_ms = iv.interval_s * 1000 if iv is not None else ds_interval_ms
    for fi, (fn, aid) in enumerate(funcs):
        for gid, ts, bits, isi in O.run_query(batch, query_of(start, end, gagg, fn, interval_ms, flags)):
            assert not isi.any()   # downsampled group results are doubles
            for t, v in zip(ts.tolist(), bits.view(np.float64).tolist()):
                assert t % 1000 == 0
                s = t // 1000
                vflags, vb = R.encode_value(v, False)
                if iv is not None:
                    base = R.basetime(s, iv)
                    qual = R.qualifier(s, base, vflags, aid, iv)
                else:
                    base = s - s % 3600
                    qual = struct.pack(">H", ((s - base) << 4) | vflags)
                out.append((fi, gid, base, qual, vb))
    return out


def check(eng, batch, interval, span, start, end, gagg="sum", funcs=FUNCS, flags=0, ds_interval_ms=0):
    from opentsdb_amd import engine
    exp = expected_cells(batch, R.Interval(interval, span) if interval else None, start, end, gagg, funcs, flags,
                         ds_interval_ms)
    eng.load(batch)
    cells = eng.preagg(engine.rollup_interval(interval, span) if interval else None, start, end, gagg, funcs, flags,
                       ds_interval_ms)
    got = [cells.cell(i) for i in range(len(cells))]
    assert len(got) == len(exp), (len(got), len(exp))
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g == e, (i, g, e)
    return got


# ---- CPU: the inputs are order-free ----------------------------------------------------------
def test_inputs_are_order_free():
    """The oracle over the mixed store and over the same series permuted within each group
    gives the same bits: sums and LERP values of these inputs do not depend on the order."""
    a = mixed_store()
    b = mixed_store(perm=[2, 0, 1, 4, 3, 5, 7, 6, 8])
    for gagg in ("sum", "zimsum", "min", "max", "mimmax", "count"):
        for fn, _ in FUNCS:
            q = query_of(MIX_START, MIX_END, gagg, fn, 600000)
            ra, rb = O.run_query(a, q), O.run_query(b, q)
            assert len(ra) == len(rb) == 3
            for (g1, t1, b1, _), (g2, t2, b2, _) in zip(ra, rb):
                assert g1 == g2 and np.array_equal(t1, t2) and np.array_equal(b1, b2), (gagg, fn, g1)
                assert not np.any(b1 == np.uint64(1 << 63))   # no -0.0


# ---- form A ------------------------------------------------------------------------------
@gpu
def test_one_series_one_group_one_bucket(eng):
    rng = np.random.default_rng(1)
    b = synth.from_series([quarter_series(rng, [T0 + 60, T0 + 120])], [0])
    got = check(eng, b, "1h", "1d", T0, T0 + 3600)
    assert len(got) == 4


@gpu
@pytest.mark.parametrize("gagg", ["sum", "min", "max", "count", "zimsum", "mimmax", "p99"])
def test_mixed_store_aggregators(eng, gagg):
    got = check(eng, mixed_store(), "10m", "1d", MIX_START, MIX_END, gagg)
    assert {c[1] for c in got} == {0, 1, 2}        # group 3 lies outside the range, -1 takes no part
    per = {g: sum(1 for c in got if c[0] == 0 and c[1] == g) for g in (0, 1, 2)}
    # groups 1 and 2 hold no data before the range: 68 slots, and slots 10..60 without slot 50 (no
    # span has a point there, so nothing is emitted: sparse emit flags)
    assert per[1] == 68 and per[2] == 50 and per[0] >= 68
    if gagg == "sum":
        assert {len(c[4]) for c in got} == {4, 8}  # float32 and float64 cells in one call


@gpu
@pytest.mark.parametrize("gagg", ["avg", "dev"])
def test_mixed_store_ordered(eng, gagg):
    got = check(eng, mixed_store(), "10m", "1d", MIX_START, MIX_END, gagg, flags=abi.QF_ORDERED)
    assert got


@gpu
def test_function_subset_and_ids(eng):
    got = check(eng, mixed_store(), "10m", "1d", MIX_START, MIX_END, "sum", (("min", 7), ("sum", 42)))
    assert {c[3][0] for c in got} == {7, 42}


@gpu
@pytest.mark.parametrize("interval,span,start,step,n", [
    ("1h", "1d", T0 + 13 * 3600, 1200, 144),              # two days from mid-day: three day rows
    ("1d", "1n", T0 + 26 * 86400, 6 * 3600, 40),          # 2013-01-27 .. 02-05: a month end
    ("6h", "1y", T0 + 362 * 86400, 2 * 3600, 72),         # 2013-12-29 .. 2014-01-03: a year end
])
def test_row_span_boundaries(eng, interval, span, start, step, n):
    b = regular_store(4, 2, start, step, n, seed=n)
    got = check(eng, b, interval, span, start, start + n * step)
    assert len({c[2] for c in got}) >= 2   # more than one row base time


@gpu
def test_many_blocks(eng):
    """4 functions x 40 groups x 100 slots = 16 000 entries: the scan spans many blocks."""
    b = regular_store(80, 40, T0, 30, 200, seed=7)
    got = check(eng, b, "1m", "1h", T0, T0 + 6000)
    assert len(got) == 4 * 40 * 100


@gpu
def test_grid_stride(eng):
    """4 functions x 1000 groups x 180 slots = 720 000 entries: more than the encode kernels'
    2048 blocks of 256 threads, so every thread strides to a second entry.  One series a group with
    a tenth of its minutes missing (sparse flags on both sides of the stride).  At this size the
    oracle's points are encoded with numpy -- the same rule, restated for hour rows and checked
    against the oracle.rollup encoder on the first and last 300 cells -- and whole arrays compared."""
    from opentsdb_amd import engine
    rng = np.random.default_rng(99)
    G, start, end = 1000, T0, T0 + 180 * 60
    minutes = np.arange(start, start + 140 * 60, 60)
    rows = [quarter_series(rng, minutes[rng.random(140) >= 0.1], big_at=(3,)) for _ in range(G)]
    b = synth.from_series(rows, list(range(G)))
    iv = R.Interval("1m", "1h")
    fi, grp, sec, val = [], [], [], []
    for i, (fn, aid) in enumerate(FUNCS):
        for gid, ts, bits, _ in O.run_query(b, query_of(start, end, "sum", fn, 60000)):
            fi.append(np.full(len(ts), i, np.int32))
            grp.append(np.full(len(ts), gid, np.int32))
            sec.append(ts // 1000)
            val.append(bits.view(np.float64))
    fi, grp, sec, val = (np.concatenate(x) for x in (fi, grp, sec, val))
    n = len(fi)
    assert n > 4 * G * 100
    base = sec - sec % 3600
    f32 = val.astype(np.float32).astype(np.float64) == val
    word = (((sec - base) // 60) << 4) | np.where(f32, 0xB, 0xF)
    qual = np.stack([np.array([a for _, a in FUNCS])[fi], word >> 8, word & 0xFF], axis=1).astype(np.uint8)
    vlen = np.where(f32, 4, 8)
    wide = np.zeros((n, 8), np.uint8)
    wide[f32, :4] = val[f32].astype(">f4").view(np.uint8).reshape(-1, 4)
    wide[~f32] = val[~f32].astype(">f8").view(np.uint8).reshape(-1, 8)
    value = wide[np.arange(8)[None, :] < vlen[:, None]]
    voff = np.concatenate([[0], np.cumsum(vlen)]).astype(np.uint64)
    for c in list(range(300)) + list(range(n - 300, n)):   # the numpy encoder against oracle.rollup
        vflags, vb = R.encode_value(float(val[c]), False)
        bt = R.basetime(int(sec[c]), iv)
        assert (bt, R.qualifier(int(sec[c]), bt, vflags, FUNCS[fi[c]][1], iv), vb) == \
            (int(base[c]), bytes(qual[c]), bytes(value[voff[c]:voff[c + 1]]))
    eng.load(b)
    cells = eng.preagg(engine.rollup_interval("1m", "1h"), start, end, "sum", FUNCS)
    assert len(cells) == n and not f32.all() and f32.any()
    np.testing.assert_array_equal(cells.func_index, fi)
    np.testing.assert_array_equal(cells.group, grp)
    np.testing.assert_array_equal(cells.base_time, base.astype(np.uint32))
    np.testing.assert_array_equal(cells.qual_off, np.arange(n + 1, dtype=np.uint64) * 3)
    np.testing.assert_array_equal(cells.qualifier.reshape(-1, 3), qual)
    np.testing.assert_array_equal(cells.val_off, voff)
    np.testing.assert_array_equal(cells.value, value)


@gpu
def test_ordered_full_mantissa(eng):
    """Full 53-bit mantissa float64 values under TSDB_QF_ORDERED, bit-exact against the oracle."""
    b = synth.generate(8, T0, 600, 10000, value_kind=4, n_groups=2)
    got = check(eng, b, "10m", "1d", T0, T0 + 6000, "sum", flags=abi.QF_ORDERED)
    assert any(len(c[4]) == 8 for c in got)


# ---- form B ------------------------------------------------------------------------------
def form_b_store():
    return regular_store(6, 3, T0 + 1800, 20, 3 * 180 + 30, seed=11)


@gpu
def test_form_b_cells(eng):
    start, end = T0 + 1800, T0 + 1800 + 3 * 3600
    got = check(eng, form_b_store(), None, None, start, end, "sum", (("sum", 0),), ds_interval_ms=60000)
    # 190 minutes of data from the start, all in hour rows the query scans (a query returns the
    # buckets of every scanned row, also past its end time): 190 cells a group, four hour rows
    assert len(got) == 3 * 190 and all(len(c[3]) == 2 for c in got)
    assert len({c[2] for c in got}) == 4


@gpu
def test_form_b_round_trip(eng):
    """The downloaded cells loaded as ordinary columns (tsdbhip_load_cells), one series per
    group: sum:1m-sum over them returns the oracle's points of the original query."""
    from tests.test_gpu_parity import assert_groups_match
    start, end = T0 + 1800, T0 + 1800 + 3 * 3600
    b = form_b_store()
    q = query_of(start, end, "sum", "sum", 60000)
    want = O.run_query(b, q)
    eng.load(b)
    cells = eng.preagg(None, start, end, "sum", (("sum", 0),), ds_interval_ms=60000)
    groups = sorted({int(g) for g in cells.group})
    assert groups == [g for g, *_ in want] == [0, 1, 2]
    series = []
    for g in groups:
        rows = {}
        for i in np.flatnonzero(cells.group == g):
            _, _, base, qual, val = cells.cell(int(i))
            rows.setdefault(base, []).append((qual, val, None))
        series.append(sorted(rows.items()))
    eng.load_cells(abi.HostCellBatch.from_rows(series, groups))
    assert_groups_match(eng.run(q), want, "sum", tol=0.0, ctx="form B round trip")


# ---- form A round trip through RollupStore and TsdbQuery -----------------------------------
@gpu
def test_form_a_round_trip(eng):
    from opentsdb_amd.query import TsdbQuery
    from opentsdb_amd.rollup_read import RollupConfig, RollupStore
    from opentsdb_amd.store import MockStore
    from opentsdb_amd import engine
    rng = np.random.default_rng(5)
    store = MockStore()
    start, end = T0, T0 + 6 * 3600
    for h in range(6):
        for t in range(start, end, 600):
            if h == 3 and t % 3600 == 1800:
                continue
            store.add_float("sys.cpu", t, float(rng.integers(1, 1 << 20)) * 0.25, {"host": f"h{h}", "colo": f"c{h % 3}"})

    def query(rollups, tags):
        q = TsdbQuery(store, runner=eng.run_batch, rollups=rollups, rollup_runner=eng.run_rollup_batch)
        q.setStartTime(start)
        q.setEndTime(end - 1)
        q.setTimeSeries("sys.cpu", tags, "sum", False)
        q.downsample("1h-sum")
        return q

    raw = query(None, {"colo": "*"})
    batch, keys = raw.build_batch()
    want = O.run_query(batch, raw.to_abi())
    assert len(want) == 3
    eng.load(batch)
    cells = eng.preagg(engine.rollup_interval("1h", "1d"), start, end, "sum", FUNCS)
    rs = RollupStore(RollupConfig({"sum": 0, "count": 1, "max": 2, "min": 3}, [("1h", "1d")]), store)
    rs.put_preagg_cells("sys.cpu", keys, ["colo"], cells, "1h", "sum")
    q = query(rs, {"colo": "*", "_aggregate": "SUM"})
    assert q.isPreAggregate() and q.tableToBeScanned() == ("rollup-agg", "1h")
    out = q.run()
    assert len(out) == len(want)
    for dp, (gid, ts, bits, _) in zip(out, want):
        assert dp.group_key == keys[gid]
        np.testing.assert_array_equal(dp.ts, ts)
        np.testing.assert_array_equal(dp.bits, bits)
    # the temporal table holds none of it
    assert query(rs, {"colo": "*"}).run() == []


# ---- refusals ----------------------------------------------------------------------------
def resident_cells(e, cap=4096):
    """Number of cells a download returns now, read into arrays of `cap` cells (the engine
    gives no count outside preagg_run): the function-index entries it wrote."""
    from opentsdb_amd import engine
    fi = np.full(cap, -7, np.int32)
    voff = np.full(cap + 1, 2 ** 63, np.uint64)
    rc = engine.lib().tsdbhip_preagg_download(e.ctx, fi.ctypes.data, None, None, None, None, voff.ctypes.data, None)
    assert rc == 0 and voff[0] == 0
    return int(np.count_nonzero(fi != -7))


def spec_of(iv, start=T0, end=T0 + 3600, gagg="sum", funcs=(("sum", 0),), flags=0, ds_interval_ms=0, n_funcs=None):
    sp = abi.PreaggSpec()
    if iv is not None:
        sp.interval = iv
    sp.ds_interval_ms = ds_interval_ms
    sp.start_s, sp.end_s = start, end
    sp.groupby_aggregator = abi.AGG[gagg] if isinstance(gagg, str) else gagg
    sp.flags = flags
    sp.n_funcs = len(funcs) if n_funcs is None else n_funcs
    for i, (fn, aid) in enumerate(funcs[:4]):
        sp.func[i] = abi.AGG[fn] if isinstance(fn, str) else fn
        sp.agg_id[i] = aid
    return sp


def run_code(e, sp):
    from opentsdb_amd import engine
    n, qb, vb = C.c_int64(), C.c_uint64(), C.c_uint64()
    return engine.lib().tsdbhip_preagg_run(e.ctx, C.byref(sp) if sp is not None else None, C.byref(n), C.byref(qb),
                                           C.byref(vb))


@gpu
def test_illegal_arguments(eng):
    from opentsdb_amd import engine
    eng.load(regular_store(2, 1, T0, 60, 60, seed=3))
    iv = engine.rollup_interval("10m", "1d")
    bad_iv = abi.RollupInterval(600, 0, b"d", b"m", 1)
    bad_units = abi.RollupInterval(600, 144, b"w", b"m", 1)
    cases = {
        "null spec": None,
        "invalid interval": spec_of(bad_iv),
        "invalid interval units": spec_of(bad_units),
        "negative interval": spec_of(abi.RollupInterval(-600, 144, b"d", b"m", 1)),
        "no function": spec_of(iv, n_funcs=0),
        "five functions": spec_of(iv, funcs=FUNCS, n_funcs=5),
        "form B two functions": spec_of(None, funcs=(("sum", 0), ("max", 0)), ds_interval_ms=60000),
        "form A avg": spec_of(iv, funcs=(("avg", 0),)),
        "form B none": spec_of(None, funcs=(("none", 0),), ds_interval_ms=60000),
        "form B unknown function": spec_of(None, funcs=((99, 0),), ds_interval_ms=60000),
        "group by none": spec_of(iv, gagg="none"),
        "group by unknown": spec_of(iv, gagg=99),
        "group by negative": spec_of(iv, gagg=-1),
        "empty range": spec_of(iv, start=T0, end=T0),
        "negative start": spec_of(iv, start=-1, end=T0),
        "unknown flag": spec_of(iv, flags=0x2),
        "form B ms interval": spec_of(None, ds_interval_ms=1500),
        "form B no interval": spec_of(None, ds_interval_ms=0),
    }
    for name, sp in cases.items():
        assert run_code(eng, sp) == abi.TSDB_E_ILLEGAL_ARGUMENT, name
    sp = spec_of(iv)
    n = C.c_int64()
    assert engine.lib().tsdbhip_preagg_run(eng.ctx, C.byref(sp), None, None, None) == abi.TSDB_E_ILLEGAL_ARGUMENT
    assert engine.lib().tsdbhip_preagg_run(None, C.byref(sp), C.byref(n), None, None) == abi.TSDB_E_ILLEGAL_ARGUMENT
    assert run_code(eng, spec_of(iv)) == 0   # and the valid spec runs


@gpu
def test_infinite_value_rejected_then_valid_call(eng):
    from opentsdb_amd import engine
    ts = (T0 + np.arange(0, 3600, 60)) * 1000
    fv = np.full(len(ts), 1.5)
    fv[7] = np.inf
    b = synth.from_series([synth.encode_rows(ts, None, fv, np.ones(len(ts), int), np.zeros(len(ts), bool))], [0])
    eng.load(b)
    iv = engine.rollup_interval("10m", "1d")
    with pytest.raises(engine.EngineError) as ei:
        eng.preagg(iv, T0, T0 + 3600, "sum", FUNCS)
    assert ei.value.code == abi.TSDB_E_ILLEGAL_ARGUMENT
    assert resident_cells(eng) == 0   # no output
    check(eng, regular_store(2, 1, T0, 60, 60, seed=3), "10m", "1d", T0, T0 + 3600)


@gpu
def test_rollup_batch_refused(eng):
    from opentsdb_amd import engine
    from opentsdb_amd.rollup_read import make_rollup_batch
    iv = engine.rollup_interval("10m", "1d")
    cell = (struct.pack(">H", (0 << 4) | 0x7), struct.pack(">q", 5))
    eng.load_rollup(make_rollup_batch([(None, [(T0, [cell], [])])], [0], iv, False))
    assert run_code(eng, spec_of(iv)) == abi.TSDB_E_NOT_IMPLEMENTED


@gpu
def test_multi_device_context_refused():
    from opentsdb_amd import engine
    md = engine.Engine(devices=[0, 0])
    try:
        md.load(regular_store(4, 2, T0, 60, 60, seed=3))
        assert run_code(md, spec_of(engine.rollup_interval("10m", "1d"))) == abi.TSDB_E_NOT_IMPLEMENTED
        assert engine.lib().tsdbhip_preagg_download(md.ctx, None, None, None, None, None, None, None) == \
            abi.TSDB_E_NOT_IMPLEMENTED
    finally:
        md.close()


@gpu
def test_rollup_run_output_undisturbed(eng):
    """A rollup_run result downloaded after a preagg_run is unchanged, and a load drops the
    pre-aggregate cells."""
    from opentsdb_amd import engine
    b = mixed_store()
    iv = engine.rollup_interval("10m", "1d")
    eng.load(b)
    nc, nb = eng.rollup_run(iv, MIX_START, MIX_END)
    before = eng.rollup_download(nc, nb)
    n, qb, vb = eng.preagg_run(iv, MIX_START, MIX_END, "sum", FUNCS)
    assert n > 0
    after = eng.rollup_download(nc, nb)
    for name in ("series", "base_time", "qualifier", "val_off", "value"):
        np.testing.assert_array_equal(getattr(before, name), getattr(after, name), err_msg=name)
    cells = eng.preagg_download(n, qb, vb)
    assert len(cells) == n and int(cells.val_off[-1]) == vb and int(cells.qual_off[-1]) == qb == 3 * n
    assert n <= 4096 and resident_cells(eng) == n
    eng.load(b)
    assert resident_cells(eng) == 0
