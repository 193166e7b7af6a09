"""Host side of regrouping the resident batch (tsdbhip_regroup, query.ResidentSpans): the
argument checks that need no device, the group ids ResidentSpans derives from a TsdbQuery's tag
filters and group-by tags against TsdbQuery.build_batch's own partition, its refusals, and the
`options` context manager restoring nested values."""
from __future__ import annotations

import numpy as np
import pytest

from opentsdb_amd import abi, engine
from opentsdb_amd.query import ResidentSpans, TsdbQuery
from opentsdb_amd.store import MockStore

T0 = 1356998400
METRIC = "sys.cpu.user"
START, END = T0, T0 + 4 * 3600   # the resident range: four hour rows

# tags of the store's 12 series; one lacks dc, the last has rows only outside the resident range
TAGS = [
    {"host": "web01", "dc": "lga"}, {"host": "web02", "dc": "lga"}, {"host": "web03", "dc": "lga"},
    {"host": "web01", "dc": "sjc"}, {"host": "web02", "dc": "sjc"}, {"host": "db01", "dc": "sjc"},
    {"host": "db02", "dc": "ams"}, {"host": "web04", "dc": "ams"}, {"host": "web05", "dc": "ams"},
    {"host": "db03", "dc": "lga"},
    {"host": "nodc01"},
    {"host": "late01", "dc": "lga"},
]
OUTSIDE = 11


def make_store():
    rng = np.random.default_rng(7)
    st = MockStore()
    for i, tags in enumerate(TAGS):
        if i == OUTSIDE:
            times = range(END + 3600, END + 7200, 600)
        elif i == 4:   # rows in the first hour only: inside the resident range, outside a later query's
            times = range(START, START + 3600, 300)
        else:
            times = range(START, END, 300)
        for t in times:
            st.add_float(METRIC, t, float(rng.integers(1, 1 << 20)) * 0.25, tags)
    return st


class FakeEngine:
    """Records what ResidentSpans hands the engine; run() returns no group."""

    def __init__(self):
        self.loaded = None
        self.regroups = []
        self.queries = []

    def load(self, batch):
        self.loaded = batch

    def regroup(self, ids):
        self.regroups.append(np.asarray(ids, np.int32).copy())

    def run(self, q):
        self.queries.append(q)
        return []


def query(store, tags, start=START, end=END - 1, ds="10m-avg", agg="sum"):
    q = TsdbQuery(store)
    q.setStartTime(start)
    q.setEndTime(end)
    q.setTimeSeries(METRIC, tags, agg, False)
    if ds:
        q.downsample(ds)
    return q


def passes(tags, qtags):
    """The tag filter, restated from the tag names: every query tag present, a literal or an
    or-list matched."""
    for k, v in qtags.items():
        if k not in tags:
            return False
        if v != "*" and tags[k] not in v.split("|"):
            return False
    return True


QUERIES = [
    {},
    {"host": "*"},
    {"dc": "*"},
    {"dc": "lga", "host": "*"},
    {"host": "web01|web02"},
    {"dc": "nowhere"},
]


@pytest.fixture(scope="module")
def store():
    return make_store()


def test_null_arguments_need_no_device():
    L = engine.lib()
    ids = np.zeros(4, np.int32)
    assert L.tsdbhip_regroup(None, ids.ctypes.data, 4) == abi.TSDB_E_ILLEGAL_ARGUMENT
    assert L.tsdbhip_regroup(None, None, 0) == abi.TSDB_E_ILLEGAL_ARGUMENT
    assert abi.GROUP_NONE == -1 and abi.GROUP_EXCLUDED == -2
    assert "tsdbhip_regroup" in engine.EXPORTS


def test_resident_load_is_the_unfiltered_scan(store):
    fe = FakeEngine()
    rs = ResidentSpans(store, METRIC, START, END, engine=fe)
    assert fe.loaded.n_series == len(TAGS) - 1 == len(rs.span_keys)   # the series outside the range has no span
    assert fe.loaded.n_rows == 10 * 4 + 1
    assert not fe.regroups


@pytest.mark.parametrize("qtags", QUERIES, ids=lambda t: ",".join(f"{k}={v}" for k, v in t.items()) or "none")
@pytest.mark.parametrize("window", ["whole", "late"])
def test_ids_reproduce_build_batch(store, qtags, window):
    """The recorded ids give build_batch's partition -- same key -> same member series, in the
    same order -- and mark exactly the series the filter rejects GROUP_EXCLUDED.  In the late
    window one resident series has no row in the query's scan range: build_batch does not see
    it, the resident store keeps it in its group (it contributes nothing)."""
    fe = FakeEngine()
    rs = ResidentSpans(store, METRIC, START, END, engine=fe)
    start = START if window == "whole" else START + 2 * 3600
    q = query(store, qtags, start=start)
    assert rs.run(q) == []
    assert len(fe.regroups) == 1 and len(fe.queries) == 1
    ids = fe.regroups[0]
    assert len(ids) == len(rs.span_keys)
    # which resident span carries which tags
    tagk = {v: k for k, v in store.tagk.ids.items()}
    tagv = {v: k for k, v in store.tagv.ids.items()}
    names = [{tagk[k]: tagv[v] for k, v in sk[1]} for sk in rs.span_keys]
    assert sorted(map(str, names)) == sorted(map(str, TAGS[:OUTSIDE]))
    excluded = {i for i, t in enumerate(names) if not passes(t, qtags)}
    assert {int(i) for i in np.flatnonzero(ids == abi.GROUP_EXCLUDED)} == excluded
    assert ids.min() >= abi.GROUP_EXCLUDED
    # build_batch's partition, from the spans its scan returned
    seen = []
    scan = store.scan
    try:
        store.scan = lambda *a: seen.append(scan(*a)) or seen[-1]
        batch, keys = q.build_batch()
    finally:
        del store.scan
    spans = seen[-1] if seen else []
    assert batch.n_series == len(spans)
    in_scan = {sk for sk, _ in spans}
    want, want_none = {}, []
    for (sk, _), g in zip(spans, batch.group_id.tolist()):
        (want.setdefault(keys[g], []) if g >= 0 else want_none).append(sk)
    _, rkeys = rs.group_ids(q)
    got, got_none = {}, []
    for sk, g in zip(rs.span_keys, ids.tolist()):
        if g == abi.GROUP_EXCLUDED or sk not in in_scan:
            continue
        (got.setdefault(rkeys[g], []) if g >= 0 else got_none).append(sk)
    assert got == want and got_none == want_none
    if window == "late" and passes(TAGS[4], qtags):
        assert len(in_scan) < len(ids) - len(excluded)   # the first-hour series: resident, not scanned
    if qtags == {"dc": "nowhere"}:
        assert not spans and len(excluded) == len(ids)
    if qtags == {"dc": "*"}:   # "*" needs the tag: the series without dc is filtered out, not ungrouped
        assert names.index({"host": "nodc01"}) in excluded and not got_none
    # group numbers are dense over the visible series
    vis = ids[ids >= 0]
    if len(vis):
        assert set(vis.tolist()) == set(range(int(vis.max()) + 1))


def test_refusals(store):
    fe = FakeEngine()
    rs = ResidentSpans(store, METRIC, START + 3600, END - 3600, engine=fe)
    with pytest.raises(ValueError, match="outside the resident range"):
        rs.run(query(store, {"host": "*"}, start=START, end=START + 3 * 3600 - 1))     # starts before it
    with pytest.raises(ValueError, match="outside the resident range"):
        rs.run(query(store, {"host": "*"}, start=START + 3600, end=END - 1))           # ends after it
    q = query(store, {"host": "*"}, start=START + 3600, end=END - 3600 - 1)
    q.setPreAggregate(True)
    assert q.tableToBeScanned()[0] == "agg"
    with pytest.raises(ValueError, match="raw-table"):
        rs.run(q)
    with pytest.raises(ValueError, match="another store or metric"):
        rs.run(query(make_store(), {"host": "*"}, start=START + 3600, end=END - 3600 - 1))
    assert not fe.regroups and not fe.queries
    with pytest.raises(ValueError, match="empty resident scan range"):
        ResidentSpans(store, METRIC, END, START, engine=fe)
    # a query whose scan range is the resident range exactly runs
    assert rs.run(query(store, {"host": "*"}, start=START + 3600, end=END - 3600 - 1, ds="1m-sum")) == []
    assert len(fe.regroups) == 1


def test_options_restore_nested_values():
    engine.reset_options()
    try:
        engine.set_option("SEQ", 1)
        with engine.options(SEQ=0, FAST=0):
            assert (engine.get_option("SEQ"), engine.get_option("FAST")) == (0, 0)
            with engine.options(SEQ=2):
                assert engine.get_option("SEQ") == 2
                with engine.options(SEQ=None):
                    assert engine.get_option("SEQ") == -1
                assert engine.get_option("SEQ") == 2
            assert (engine.get_option("SEQ"), engine.get_option("FAST")) == (0, 0)
            with pytest.raises(RuntimeError):
                with engine.options(FAST=1):
                    raise RuntimeError("the block fails")
            assert engine.get_option("FAST") == 0
        assert (engine.get_option("SEQ"), engine.get_option("FAST")) == (1, -1)
    finally:
        engine.reset_options()
