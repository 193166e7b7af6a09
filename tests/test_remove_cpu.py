"""Host side of removing rows from the resident batch (tsdbhip_remove, query.ResidentSpans.delete /
refresh(remove_missing=True) / retire_empty, store.MockStore.delete_rows): the expectation builder
remove_batch against stores built from full point lists, what ResidentSpans hands the engine and
keeps, and the argument checks that need no device."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

from opentsdb_amd import abi, engine, synth
from opentsdb_amd.query import ResidentSpans
from tests.append_util import batches_equal, merge_batches, split
from tests.remove_util import remove_batch
from tests.test_append_cpu import store_points
from tests.test_regroup_cpu import END, METRIC, QUERIES, START, FakeEngine, make_store, passes, query
from tests.trim_util import trim_batch

T0 = 1356998400
H = 3600
GIDS = [0, 1, -1, 0, abi.GROUP_EXCLUDED, 2]
ALL = (0, 1 << 32)


def hour(k):
    return (T0 + k * H, T0 + (k + 1) * H)


def without(p, hours):
    """The rows of Points p with the given hours' points left out."""
    rows = []
    for k in range(3):
        if k not in hours:
            rows += p.rows(*hour(k))
    return rows


@pytest.mark.parametrize("gone", [{0: [0]}, {1: [1]}, {2: [2]}, {3: [0, 2]}, {0: [1], 4: [0, 1], 5: [2]}, {2: [0, 1, 2]}, {}])
@pytest.mark.parametrize("drop", [False, True])
def test_remove_equals_the_store_without_those_hours(gone, drop):
    """gone: series -> hours whose rows go.  What stays is the store built from the point lists
    with those hours' points left out; with drop_empty a series left without a point is not in it."""
    pts = store_points()
    full = synth.from_series([p.rows() for p in pts], GIDS)
    ranges = [(s, *hour(k)) for s, hs in gone.items() for k in hs]
    stays = [s for s in range(len(pts)) if not (drop and len(gone.get(s, [])) == 3)]
    want = synth.from_series([without(pts[s], gone.get(s, [])) for s in stays], [GIDS[s] for s in stays])
    got, new_index = remove_batch(full, ranges, drop)
    batches_equal(got, want)
    assert new_index.tolist() == [stays.index(s) if s in stays else -1 for s in range(len(pts))]
    if not drop:
        assert new_index.tolist() == list(range(len(pts))) and got.group_id.tolist() == GIDS


def test_ranges_compose_overlap_and_may_be_empty():
    pts = store_points()
    full = synth.from_series([p.rows() for p in pts], GIDS)
    r1 = [(0, *hour(0)), (3, T0, T0 + 2 * H), (5, *ALL)]
    r2 = [(3, T0 + H, T0 + 3 * H), (0, *hour(0)), (1, T0 + H, T0 + H + 1), (3, T0 + H, T0 + 3 * H)]
    for drop in (False, True):
        u, ux = remove_batch(full, r1 + r2, drop)
        a, ax = remove_batch(full, r1, False)
        b, _ = remove_batch(a, r2, drop)
        batches_equal(b, u)                                            # remove(R1); remove(R2) == remove(R1 u R2)
        batches_equal(remove_batch(full, r2 + r1, drop)[0], u)         # in any order
        again = [(int(ux[i]), lo, hi) for i, lo, hi in r1 + r2 if ux[i] >= 0]
        v, vx = remove_batch(u, again, drop)                           # idempotent
        batches_equal(v, u)
        assert vx.tolist() == list(range(u.n_series))
    assert ux.tolist() == [0, 1, 2, -1, 3, -1]
    # ranges that match no row: between two rows, past the last, before the first, from == to, a row-less series
    empty = [(0, T0 + 1, T0 + H), (1, T0 + 3 * H, T0 + 9 * H), (2, 0, T0), (4, T0 + H, T0 + H)]
    e, ex = remove_batch(full, empty, True)
    batches_equal(e, full)
    assert ex.tolist() == list(range(6))
    rowless, _ = remove_batch(full, [(2, *ALL)], False)
    assert int(np.diff(rowless.series_row_ptr)[2]) == 0
    batches_equal(remove_batch(rowless, [(2, *ALL), (2, *hour(1))], False)[0], rowless)
    d, dx = remove_batch(rowless, [], True)                            # "retire what was emptied"
    assert dx.tolist() == [0, 1, -1, 2, 3, 4] and d.n_series == 5 and d.group_id.tolist() == [0, 1, 0, abi.GROUP_EXCLUDED, 2]


@pytest.mark.parametrize("cutoff", [T0 - 1, T0, T0 + H, T0 + H + 1700, T0 + 2 * H, T0 + 9 * H])
def test_remove_of_every_prefix_is_a_trim(cutoff):
    pts = store_points()
    full = synth.from_series([p.rows() for p in pts], GIDS)
    got, idx = remove_batch(full, [(s, 0, cutoff) for s in range(len(pts))], False)
    batches_equal(got, trim_batch(full, cutoff))
    assert idx.tolist() == list(range(len(pts)))


@pytest.mark.parametrize("where", ["first", "middle", "last", "none"])
def test_remove_undoes_an_inserting_delta(where):
    """A delta that only inserts -- a cut on the hour, and a new series first, in the middle or last --
    and then the remove of exactly its rows, with drop_empty for the new series."""
    pts = store_points()
    resident = [True] * len(pts)
    if where != "none":
        resident[{"first": 0, "middle": 3, "last": len(pts) - 1}[where]] = False
    a, d, idx, new, full = split(pts, GIDS, T0 + 2 * H, resident=resident)
    m = merge_batches(a, d, idx, new)
    batches_equal(m, full)
    ranges = []
    for i, s in enumerate(idx):
        for r in range(int(d.series_row_ptr[i]), int(d.series_row_ptr[i + 1])):
            ranges.append((int(s), int(d.row_base_time[r]), int(d.row_base_time[r]) + 1))
    got, nx = remove_batch(m, ranges, True)
    batches_equal(got, a)
    assert [i for i, x in enumerate(nx) if x < 0] == [i for i, r in enumerate(resident) if not r]


# ---- MockStore.delete_rows ----------------------------------------------------------------------
@pytest.mark.parametrize("qtags", QUERIES[:5])
def test_delete_rows_deletes_what_the_scan_returns(qtags):
    st = make_store()
    q = query(st, qtags, start=START + H, end=START + 3 * H - 1)
    pred = q._filters()[0]
    s, e = q.scan_bounds()
    scanned = [(sk, r[0]) for sk, rows in st.scan(METRIC, s, e, pred) for r in rows]
    others = st.scan(METRIC, 0, 1 << 32, lambda tags: not pred(tags))
    n_before = len(st.rows)
    gone = st.delete_rows(METRIC, s, e, pred)
    assert gone == scanned and len(gone) > 0
    assert st.scan(METRIC, s, e, pred) == [] and len(st.rows) == n_before - len(gone)
    assert st.scan(METRIC, 0, 1 << 32, lambda tags: not pred(tags)) == others
    assert all(not (s <= b < e) for sk, rows in st.scan(METRIC, 0, 1 << 32, pred) for b, _, _ in rows)
    assert st.delete_rows(METRIC, s, e, pred) == []                  # idempotent


# ---- ResidentSpans.delete / refresh(remove_missing) / retire_empty ------------------------------
class RemoveEngine(FakeEngine):
    """Records the removes and answers them as remove_batch would (new_index only)."""

    def __init__(self):
        super().__init__()
        self.removes = []
        self.upserts = []
        self.rows = None     # [series] row count, kept up to date

    def load(self, batch):
        super().load(batch)
        self.rows = np.diff(batch.series_row_ptr).tolist()
        self.bases = [batch.row_base_time[int(batch.series_row_ptr[i]):int(batch.series_row_ptr[i + 1])].astype(np.int64).tolist()
                      for i in range(batch.n_series)]

    def remove(self, ranges, drop_empty=False, pack_dead_pct=abi.TRIM_NO_PACK):
        ranges = list(ranges)
        self.removes.append((ranges, drop_empty, pack_dead_pct))
        info = abi.RemoveInfo()
        for i, lo, hi in ranges:
            keep = [b for b in self.bases[i] if not lo <= b < hi]
            info.rows_removed += len(self.bases[i]) - len(keep)
            self.bases[i] = keep
        stays = [bool(b) or not drop_empty for b in self.bases]
        new_index = np.where(stays, np.cumsum(stays) - 1, -1)
        info.series_dropped = stays.count(False)
        self.bases = [b for b, s in zip(self.bases, stays) if s]
        return info, new_index

    def upsert(self, delta, series_index, series_new):
        self.upserts.append((delta, list(series_index), list(series_new)))
        return abi.UpsertInfo()


def spans_of(store):
    return store.scan(METRIC, START, END)


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("qtags", QUERIES)
def test_resident_spans_delete(qtags, drop):
    st = make_store()
    fe = RemoveEngine()
    rs = ResidentSpans(st, METRIC, START, END, engine=fe)
    keys = list(rs.span_keys)
    q = query(st, qtags, start=START + H, end=START + 3 * H - 1)
    s, e = q.scan_bounds()
    before = spans_of(st)
    out, info = rs.delete(q, drop_empty=drop)
    assert out == [] and isinstance(info, abi.RemoveInfo)
    assert len(fe.queries) == 1                                          # answered as run answers it, first
    (ranges, d, pack), = fe.removes
    assert (d, pack) == (drop, 50)
    # one range per matching resident series, over the query's scan bounds
    match = [i for i, sk in enumerate(keys) if (q._filters() is not None and q._filters()[0](sk[1]))]
    assert ranges == [(i, s, e) for i in match]
    if qtags != {"dc": "nowhere"}:                                     # (restated from the tag names)
        tagv = {v: k for k, v in st.tagv.ids.items()}
        tagk = {v: k for k, v in st.tagk.ids.items()}
        assert match == [i for i, sk in enumerate(keys) if passes({tagk[k]: tagv[v] for k, v in sk[1]}, qtags)]
    # the store lost exactly those rows, and the spans equal a fresh scan of it (row-less ones kept unless dropped)
    after = dict(spans_of(st))
    for i, (sk, rows) in enumerate(before):
        want = [r for r in rows if not (i in match and s <= r[0] < e)]
        assert after.get(sk, []) == want
    if drop:
        assert rs.spans == spans_of(st) and rs.span_keys == [sk for sk, _ in spans_of(st)]
    else:
        assert rs.span_keys == keys and rs.spans == [(sk, after.get(sk, [])) for sk in keys]
    fresh = ResidentSpans(st, METRIC, START, END, engine=RemoveEngine())
    assert [sp for sp in rs.spans if sp[1]] == fresh.spans


def test_resident_spans_delete_refusals_hand_nothing_over():
    st = make_store()
    fe = RemoveEngine()
    rs = ResidentSpans(st, METRIC, START + H, END, engine=fe)
    n = len(st.rows)
    with pytest.raises(ValueError, match="outside the resident range"):
        rs.delete(query(st, {"host": "*"}, start=START, end=END - 1))
    other = make_store()
    with pytest.raises(ValueError, match="another store"):
        rs.delete(query(other, {"host": "*"}, start=START + H, end=END - 1))
    assert fe.removes == [] and len(st.rows) == n and len(other.rows) == n


def test_refresh_remove_missing_and_retire_empty():
    st = make_store()
    fe = RemoveEngine()
    rs = ResidentSpans(st, METRIC, START, END, engine=fe)
    keys = list(rs.span_keys)
    # behind the resident spans' back: hour 2 of two series goes, series 4 (first hour only) goes entirely
    pred = lambda tags: dict(tags) in ({st.tagk.ids["host"]: st.tagv.ids["web01"], st.tagk.ids["dc"]: st.tagv.ids["lga"]},   # noqa: E731
                                       {st.tagk.ids["host"]: st.tagv.ids["db01"], st.tagk.ids["dc"]: st.tagv.ids["sjc"]})
    gone = st.delete_rows(METRIC, START + 2 * H, START + 3 * H, pred)
    (only_first,) = [sk for sk, rows in rs.spans if len(rows) == 1]
    gone += st.delete_rows(METRIC, START, START + H, lambda tags: tags == only_first[1])
    assert len(gone) == 3
    with pytest.raises(ValueError, match="an upsert cannot remove rows, reload the resident spans"):
        rs.refresh(START, END)                                           # the default is unchanged
    assert fe.removes == [] and fe.upserts == []
    rs.refresh(START, END, remove_missing=True)
    (ranges, drop, pack), = fe.removes
    assert (drop, pack) == (False, abi.TRIM_NO_PACK)
    assert sorted(ranges) == sorted((keys.index(sk), b, b + 1) for sk, b in gone)
    assert len(fe.upserts) == 1                                          # then the upsert runs
    after = dict(spans_of(st))
    assert rs.span_keys == keys and rs.spans == [(sk, after.get(sk, [])) for sk in keys]
    info = rs.retire_empty()
    assert fe.removes[-1] == ([], True, abi.TRIM_NO_PACK) and info.series_dropped == 1
    assert rs.spans == spans_of(st) and only_first not in rs.span_keys
    # nothing missing: remove_missing hands the engine no remove
    rs.refresh(START, END, remove_missing=True)
    assert len(fe.removes) == 2 and len(fe.upserts) == 2


# ---- the C entry points without a device ----------------------------------------------------------
def test_export_and_illegal_arguments_need_no_device():
    assert "tsdbhip_remove" in engine.EXPORTS
    L = engine.lib()
    info = abi.RemoveInfo()
    IA = abi.TSDB_E_ILLEGAL_ARGUMENT
    r = (abi.RemoveRange * 1)(abi.RemoveRange(0, T0, T0 + H))
    assert L.tsdbhip_remove(None, None, 0, 0, abi.TRIM_NO_PACK, None, C.byref(info)) == IA
    assert L.tsdbhip_remove(None, C.cast(r, C.c_void_p), 1, abi.REMOVE_DROP_EMPTY, 0, None, None) == IA
    assert abi.REMOVE_DROP_EMPTY == 1
    assert L.tsdbhip_abi_version() == 12


def header_fields(hdr, name):
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    ctypes_of = {"int64_t": C.c_int64, "uint64_t": C.c_uint64, "int32_t": C.c_int32}
    return [(n, ctypes_of[t]) for n, t in fields]


def test_remove_structs_match_the_header():
    """abi.RemoveInfo's and abi.RemoveRange's fields, in order and by type, are the header's."""
    import os
    hdr = open(os.path.join(os.path.dirname(engine.HERE), "include", "tsdbhip.h")).read()
    assert header_fields(hdr, "tsdbhip_remove_info") == list(abi.RemoveInfo._fields_)
    assert header_fields(hdr, "tsdbhip_remove_range") == list(abi.RemoveRange._fields_)
    assert C.sizeof(abi.RemoveInfo) == 96 and C.sizeof(abi.RemoveRange) == 24
    assert "#define TSDB_REMOVE_DROP_EMPTY 1u" in hdr
    assert "#define TSDBHIP_ABI_VERSION 12" in hdr or engine.lib().tsdbhip_abi_version() == 12
