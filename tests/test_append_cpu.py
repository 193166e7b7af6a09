"""Host side of appending to the resident batch (tsdbhip_append, query.ResidentSpans.extend):
the expectation builder merge_batches against stores built from full point lists, the delta and
indices ResidentSpans.extend hands the engine, and the argument checks that need no device."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from opentsdb_amd import abi, engine
from opentsdb_amd.query import ResidentSpans
from opentsdb_amd.store import MockStore, make_batch
from tests.append_util import batches_equal, int_points, merge_batches, quarter_points, split
from tests.test_regroup_cpu import END, METRIC, START, TAGS, FakeEngine, make_store

T0 = 1356998400


def store_points(n=6, hours=3, step=300):
    rng = np.random.default_rng(11)
    pts = []
    for i in range(n):
        ts = T0 + np.arange(0, hours * 3600, step)
        pts.append(int_points(rng, ts, -100, 30000) if i % 2 else quarter_points(rng, ts))
    return pts


CUT = T0 + 2 * 3600 + 1500   # 25 minutes into the third hour


@pytest.mark.parametrize("where", ["first", "middle", "last", "none"])
def test_merge_equals_the_full_store(where):
    """A = the points before a cut inside an hour, D = the points from that hour's start on:
    merge_batches(A, D) is from_series(all points), array for array; a new series inserted first,
    in the middle and last."""
    pts = store_points()
    gids = [i % 3 for i in range(len(pts))]
    resident = [True] * len(pts)
    if where != "none":
        resident[{"first": 0, "middle": 3, "last": len(pts) - 1}[where]] = False
    a, d, idx, new, full = split(pts, gids, CUT, resident=resident)
    assert a.n_series == len(pts) - (where != "none") and int(new.sum()) == (where != "none")
    assert a.n_rows == 3 * a.n_series and d.n_rows == d.n_series + 2 * int(new.sum())
    batches_equal(merge_batches(a, d, idx, new), full)


def test_merge_series_without_delta_and_new_hour_only():
    pts = store_points()
    gids = [0, 1, -1, 0, 1, 2]
    # series 2 and 4 get nothing from the rescan
    a, d, idx, new, full = split(pts, gids, CUT, delta=[True, True, False, True, False, True])
    assert d.n_series == 4 and idx.tolist() == [0, 1, 3, 5]
    batches_equal(merge_batches(a, d, idx, new), full)
    # a cut on the hour: the delta is only a new hour row, nothing is replaced
    a, d, idx, new, full = split(pts, gids, T0 + 2 * 3600)
    assert a.n_rows == 2 * len(pts) and d.n_rows == len(pts)
    assert not set(a.row_base_time.tolist()) & set(d.row_base_time.tolist())
    batches_equal(merge_batches(a, d, idx, new), full)


def test_merge_replaces_by_base_and_keeps_resident_ids():
    pts = store_points(4)
    a, d, idx, new, full = split(pts, [0, abi.GROUP_EXCLUDED, 1, -1], CUT, resident=[True, True, False, True])
    m = merge_batches(a, d, idx, new)
    assert m.group_id.tolist() == [0, abi.GROUP_EXCLUDED, 1, -1]
    # the live hour's row is the delta's (longer) one
    r = int(m.series_row_ptr[0]) + 2
    assert int(m.row_qual_off[r + 1] - m.row_qual_off[r]) == 2 * 12
    ra = int(a.series_row_ptr[0]) + 2
    assert int(a.row_qual_off[ra + 1] - a.row_qual_off[ra]) == 2 * 5


# ---- ResidentSpans.extend ---------------------------------------------------------------------
class AppendEngine(FakeEngine):
    def __init__(self):
        super().__init__()
        self.appends = []

    def append(self, delta, series_index, series_new):
        self.appends.append((delta, np.asarray(series_index, np.int64).copy(), np.asarray(series_new, bool).copy()))
        return abi.AppendInfo()


def growing_store(until):
    """tests/test_regroup_cpu.py's store as it stood at `until`: only the points before it."""
    full = make_store()
    st = MockStore()
    st.metrics, st.tagk, st.tagv = full.metrics, full.tagk, full.tagv
    for (m, t, base), row in full.rows.items():
        for q in row.order:
            off = (int.from_bytes(q, "big") >> 4)
            if base + off < until:
                r = st.rows.setdefault((m, t, base), type(row)())
                r.cells[q] = row.cells[q]
                r.order.append(q)
    return st, full


def test_extend_hands_the_engine_the_rescan_delta():
    cut = START + 2 * 3600 + 1500
    st, full = growing_store(cut)
    fe = AppendEngine()
    rs = ResidentSpans(st, METRIC, START, START + 3 * 3600, engine=fe)   # (the live hour's row is partial)
    n_before, keys_before = len(rs.spans), set(rs.span_keys)
    assert n_before == len(TAGS) - 1 and fe.loaded.n_rows == 10 * 3 + 1
    # time moves on: the store now holds everything, one more series included
    st.rows = full.rows
    with pytest.raises(ValueError, match="cannot shrink"):
        rs.extend(START + 3 * 3600 - 1)
    rs.extend(END + 7200)
    assert rs.scan_end_s == END + 7200 and len(fe.appends) == 1
    delta, idx, new = fe.appends[0]
    fresh = ResidentSpans(full, METRIC, START, END + 7200, engine=FakeEngine())
    assert rs.span_keys == fresh.span_keys and rs.spans == fresh.spans
    # the delta is the scan from the live hour on, in SpanCmp order
    want = full.scan(METRIC, START + 2 * 3600, END + 7200)
    batches_equal(delta, make_batch(want, [abi.GROUP_EXCLUDED] * len(want)))
    assert (delta.group_id == abi.GROUP_EXCLUDED).all()
    assert idx.tolist() == [fresh.span_keys.index(sk) for sk, _ in want]
    assert new.tolist() == [sk not in keys_before for sk, _ in want]
    assert int(new.sum()) == 1 and len(fresh.spans) == n_before + 1
    # and the merged batch is the fresh resident's batch
    m = merge_batches(fe.loaded, delta, idx, new)
    batches_equal(m, make_batch(fresh.spans, m.group_id.tolist()))
    # a second extend with nothing new: an empty or pure-replacement delta, spans unchanged
    rs.extend(END + 7200)
    assert rs.spans == fresh.spans and len(fe.appends) == 2


def test_extend_from_a_given_hour():
    st, full = growing_store(START + 3600)
    fe = AppendEngine()
    rs = ResidentSpans(st, METRIC, START, START + 3600, engine=fe)
    st.rows = full.rows
    rs.extend(END, rescan_from_s=START + 3600)   # the first hour is complete: no replacement
    delta, idx, new = fe.appends[0]
    assert START not in delta.row_base_time.tolist()
    assert rs.spans == ResidentSpans(full, METRIC, START, END, engine=FakeEngine()).spans


# ---- the C entry point without a device ---------------------------------------------------------
def test_export_and_null_arguments_need_no_device():
    assert "tsdbhip_append" in engine.EXPORTS
    assert "APPEND_RESERVE" in engine.OPTIONS
    L = engine.lib()
    d = make_batch([], [])
    idx = np.zeros(1, np.int64)
    new = np.zeros(1, np.uint8)
    info = abi.AppendInfo()
    assert L.tsdbhip_append(None, C.byref(d.c), idx.ctypes.data, new.ctypes.data, C.byref(info)) == abi.TSDB_E_ILLEGAL_ARGUMENT
    assert L.tsdbhip_append(None, None, None, None, None) == abi.TSDB_E_ILLEGAL_ARGUMENT
    assert C.sizeof(abi.AppendInfo) == 64
    assert L.tsdbhip_abi_version() == 12
