"""Host side of tsdbhip_regroup_tags, no device: the plain-Python expectation
(tests/tags_ref.py) against ResidentSpans.group_ids for the old `tags` forms, the primitives'
truth table, the 2.x filter types' match answers (tests/golden/tag_filters.json, transcribed as
data from the reference's TestTagV*Filter cases), findGroupBys, what ResidentSpans(device_tags=True)
hands an engine, and the plumbing (exports, option, header, struct sizes, symbols)."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import pytest

from opentsdb_amd import abi, engine
from opentsdb_amd.query import ResidentSpans, TagVFilter, TsdbQuery
from opentsdb_amd.store import MockStore
from tests import tags_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = 1356998400
START, END = T0, T0 + 2 * 3600
METRIC = "m"


def random_store(seed, n=40):
    """Series over three tagks; some lack dc, some lack rack, host values repeat across dcs."""
    rng = np.random.default_rng(seed)
    st = MockStore()
    seen = set()
    while len(seen) < n:
        tags = {"host": f"h{rng.integers(0, 12):02d}"}
        if rng.random() < 0.8:
            tags["dc"] = ["lga", "sjc", "ams", "LGA"][rng.integers(0, 4)]
        if rng.random() < 0.5:
            tags["rack"] = f"r{rng.integers(0, 3)}"
        key = tuple(sorted(tags.items()))
        if key in seen:
            continue
        seen.add(key)
        st.add_long(METRIC, START + 60 * int(rng.integers(0, 100)), int(rng.integers(0, 100)), tags)
    return st


def query(store, tags, filters=(), explicit=False):
    q = TsdbQuery(store)
    q.setStartTime(START)
    q.setEndTime(END - 1)
    q.setTimeSeries(METRIC, tags, "sum", False)
    if filters or explicit:
        q.setFilters(list(filters), explicit_tags=explicit)
    return q


class RecordingEngine:
    """What ResidentSpans hands the engine; regroup_tags answers from tags_ref over the loaded table."""

    def __init__(self):
        self.calls = []
        self.table = None
        self.n_loaded = 0

    def load(self, batch):
        self.calls.append(("load", batch.n_series))
        self.n_loaded = batch.n_series
        self.table = None

    def load_tags(self, tag_ptr, tagk, tagv):
        assert len(tag_ptr) == self.n_loaded + 1
        self.table = [[(int(tagk[e]), int(tagv[e])) for e in range(tag_ptr[i], tag_ptr[i + 1])] for i in range(len(tag_ptr) - 1)]
        self.calls.append(("load_tags", len(self.table)))

    def regroup_tags(self, q, group_by=(), explicit_tags=False, dry=False):
        assert self.table is not None, "regroup_tags without a table"
        self.calls.append(("regroup_tags", q))
        ids, keys = TR.group_ids(self.table, q)
        return np.asarray(ids, np.int32), keys, None

    def regroup(self, ids):
        self.calls.append(("regroup", list(ids)))

    def run(self, q):
        return []

    def upsert(self, delta, series_index, series_new):
        self.calls.append(("upsert", delta.n_series))
        if any(series_new):
            self.n_loaded += sum(1 for x in series_new if x)
            self.table = None
        return abi.UpsertInfo()

    append = upsert

    def remove(self, ranges, drop_empty=False, pack_dead_pct=-1):
        self.calls.append(("remove", drop_empty))
        gone = int(np.sum(np.asarray(self.new_index) < 0))
        if gone:
            self.n_loaded -= gone
            self.table = None
        return abi.RemoveInfo(), self.new_index


def table_of(rs):
    return [list(sk[1]) for sk in rs.span_keys]


# ---- the reference against the host path ---------------------------------------------------------
OLD_FORMS = [{}, {"host": "*"}, {"dc": "*"}, {"dc": "lga", "host": "*"}, {"host": "h01|h02|nope"}, {"dc": "nowhere"},
             {"dc": "*", "rack": "*"}, {"rack": "r1", "dc": "lga|sjc"}, {"nokey": "*"}, {"dc": "a|b"}]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ref_equals_host_group_ids_for_old_tags(seed):
    st = random_store(seed)
    rs = ResidentSpans(st, METRIC, START, END, engine=RecordingEngine())
    for tags in OLD_FORMS:
        q = query(st, tags)
        ids, keys = rs.group_ids(q)
        tq = q.tag_query()
        if tq is None:
            assert set(ids) == {abi.GROUP_EXCLUDED} and keys == []
            continue
        rids, rkeys = TR.group_ids(table_of(rs), tq)
        assert rids == list(ids), tags
        assert rkeys == (list(keys) if tq.group_by_list else ([()] if any(i >= 0 for i in rids) else [])), tags


def test_old_tags_become_primitives():
    st = random_store(5)
    k, v = st.tagk.ids, st.tagv.ids
    tq = query(st, {"dc": "*", "host": "h01|h02|nope", "rack": "r1"}).tag_query()
    assert sorted(tq.filter_list) == sorted([(k["dc"], abi.TF_ANY, []), (k["host"], abi.TF_IN, sorted([v["h01"], v["h02"]])),
                                             (k["rack"], abi.TF_IN, [v["r1"]])])
    assert tq.group_by_list == sorted([k["dc"], k["host"]]) and tq.explicit_tags is False
    assert query(st, {"dc": "nowhere"}).tag_query() is None and query(st, {"nokey": "*"}).tag_query() is None


# ---- the primitives' truth table -----------------------------------------------------------------
K, OTHER = 7, 9


@pytest.mark.parametrize("kind,values,present_in,present_out,missing", [
    (TR.ANY, [], True, True, False),
    (TR.IN, [5], True, False, False),
    (TR.IN, [], False, False, False),        # an empty set matches nobody
    (TR.NOT_IN, [5], False, True, True),
    (TR.NOT_IN, [], True, True, True),       # an empty set matches everybody
    (TR.NOT_KEY, [], False, False, True),
])
def test_primitive_truth_table(kind, values, present_in, present_out, missing):
    assert TR.holds(kind, {K: 5}, K, set(values)) is present_in
    assert TR.holds(kind, {K: 6}, K, set(values)) is present_out
    assert TR.holds(kind, {OTHER: 5}, K, set(values)) is missing
    rows = [[(K, 5)], [(K, 6)], [(OTHER, 5)]]
    ids, _ = TR.group_ids(rows, ([(K, kind, values)], [], False))
    assert ids == [0 if x else abi.GROUP_EXCLUDED for x in (present_in, present_out, missing)]


def test_two_filters_on_one_tagk_and_explicit_tags():
    rows = [[(K, 5)], [(K, 6)], [(K, 7)], []]
    ids, _ = TR.group_ids(rows, ([(K, TR.IN, [5, 6]), (K, TR.NOT_IN, [6])], [], False))
    assert ids == [0, -2, -2, -2]
    # explicit_tags: a missing, an exact and an extra tag; NOT_KEY's tagk is not asked for
    rows = [[(K, 5)], [(K, 5), (OTHER, 1)], [(K, 5), (OTHER, 1), (11, 2)], [(OTHER, 1)]]
    f = [(K, TR.ANY, []), (OTHER, TR.IN, [1]), (12, TR.NOT_KEY, [])]
    assert TR.group_ids(rows, (f, [], True))[0] == [-2, 0, -2, -2]
    assert TR.group_ids(rows, (f, [], False))[0] == [-2, 0, 0, -2]
    # keys: unsigned order, NONE for a visible series that lacks a group-by tag
    rows = [[(K, 0x80000000)], [(K, 1)], [(OTHER, 3)], [(K, 0xFFFFFFFF)], [(K, 1), (OTHER, 2)]]
    ids, keys = TR.group_ids(rows, ([], [K], False))
    assert ids == [1, 0, -1, 2, 0] and keys == [(1,), (0x80000000,), (0xFFFFFFFF,)]
    assert TR.counters(ids) == (5, 0, 1, 3)


# ---- the filter types' match answers -------------------------------------------------------------
def golden_cases():
    with open(os.path.join(ROOT, "tests", "golden", "tag_filters.json"), encoding="utf-8") as f:
        return json.load(f)["cases"]


def test_filter_types_match_as_the_reference():
    cases = golden_cases()
    assert {c["type"] for c in cases} == set(["literal_or", "iliteral_or", "not_literal_or", "not_iliteral_or", "wildcard",
                                              "iwildcard", "regexp", "not_key"])
    assert sum(1 for c in cases if c["tagk"] not in c["tags"]) >= 8   # missing-tag cases
    for c in cases:
        f = TagVFilter(c["type"], c["tagk"], c["filter"])
        assert f.match(c["tags"]) is c["expected"], c


def test_filter_types_resolve_to_the_same_verdict():
    """Each golden case through tag_query(): the primitives over UID sets give match()'s answer for
    the series (with the tagk's presence asked for, as the row key regex asks)."""
    for c in golden_cases():
        st = MockStore()
        st.add_long(METRIC, START, 1, c["tags"])
        st.add_long(METRIC, START, 1, {c["tagk"]: "zzz-other", "pad": "x"})   # (every name known)
        q = query(st, {}, [{"type": c["type"], "tagk": c["tagk"], "filter": c["filter"]}])
        tq = q.tag_query()
        rs = ResidentSpans(st, METRIC, START, END, engine=RecordingEngine())
        i = [dict(sk[1]) for sk in rs.span_keys].index({st.tagk.ids[k]: st.tagv.ids[v] for k, v in c["tags"].items()})
        want = c["expected"] and (c["type"] == "not_key" or c["tagk"] in c["tags"])
        assert (TR.group_ids(table_of(rs), tq)[0][i] != abi.GROUP_EXCLUDED) is want, c
        assert (rs.group_ids(q)[0][i] != abi.GROUP_EXCLUDED) is want, c


def test_filter_constructor_refusals():
    for args in [("literal_or", "host", ""), ("literal_or", "host", "|"), ("wildcard", "host", "literal"), ("regexp", "host", ""),
                 ("not_key", "host", "x"), ("nosuch", "host", "a"), ("literal_or", "", "a")]:
        with pytest.raises(ValueError):
            TagVFilter(*args)


# ---- findGroupBys -------------------------------------------------------------------------------
def test_find_group_bys():
    st = random_store(9)
    k, v = st.tagk.ids, st.tagv.ids
    rs = ResidentSpans(st, METRIC, START, END, engine=RecordingEngine())
    # a group-by tagk also filtered by a literal: grouped once, both filters ANDed
    q = query(st, {}, [{"type": "wildcard", "tagk": "dc", "filter": "*", "groupBy": True},
                       {"type": "literal_or", "tagk": "dc", "filter": "lga|sjc", "groupBy": False}])
    tq = q.tag_query()
    assert tq.group_by_list == [k["dc"]]
    assert sorted(tq.filter_list) == sorted([(k["dc"], abi.TF_ANY, []), (k["dc"], abi.TF_IN, sorted([v["lga"], v["sjc"]]))])
    ids, keys = TR.group_ids(table_of(rs), tq)
    assert keys == sorted((v[x],) for x in ("lga", "sjc")) and (list(ids), keys) == tuple(map(list, rs.group_ids(q)))
    # a group-by on a tagk some series lack, with no filter asking for it (not_literal_or on another tagk
    # keeps them visible): those series are ungrouped
    q = query(st, {}, [{"type": "not_key", "tagk": "rack", "filter": "", "groupBy": False},
                       {"type": "iliteral_or", "tagk": "host", "filter": "H01|h02|H03", "groupBy": True}])
    tq = q.tag_query()
    assert tq.group_by_list == [k["host"]] and (k["rack"], abi.TF_NOT_KEY, []) in tq.filter_list
    tq2 = abi.HostTagQuery(tq.filter_list, [k["dc"]], False)
    ids2, _ = TR.group_ids(table_of(rs), tq2)
    assert abi.GROUP_NONE in ids2 and any(i >= 0 for i in ids2)
    # no group-by: one group
    q = query(st, {}, [{"type": "regexp", "tagk": "host", "filter": "^h0[0-4]$"}])
    tq = q.tag_query()
    assert tq.group_by_list == []
    ids, keys = TR.group_ids(table_of(rs), tq)
    assert set(ids) == {0, abi.GROUP_EXCLUDED} and keys == [()]
    assert list(ids) == list(rs.group_ids(q)[0])
    # case-insensitive literals pick every spelling: LGA and lga are two tagvs, two groups
    q = query(st, {}, [{"type": "iliteral_or", "tagk": "dc", "filter": "Lga", "groupBy": True}])
    tq = q.tag_query()
    assert tq.filter_list == [(k["dc"], abi.TF_IN, sorted([v["lga"], v["LGA"]]))]
    # not_literal_or asks for the tagk beside the NOT_IN; explicit_tags travels
    q = query(st, {}, [{"type": "not_literal_or", "tagk": "dc", "filter": "lga"}], explicit=True)
    tq = q.tag_query()
    assert tq.filter_list == [(k["dc"], abi.TF_NOT_IN, [v["lga"]]), (k["dc"], abi.TF_ANY, [])] and tq.explicit_tags is True
    ids, _ = TR.group_ids(table_of(rs), tq)
    for i, sk in zip(ids, rs.span_keys):
        d = dict(sk[1])
        assert (i == 0) == (set(d) == {k["dc"]} and d[k["dc"]] != v["lga"])
    assert list(ids) == list(rs.group_ids(q)[0])


def test_build_batch_honours_filters():
    st = random_store(11)
    q = query(st, {"dc": "*"}, [{"type": "wildcard", "tagk": "host", "filter": "h0*"}])
    batch, keys = q.build_batch()
    want = [sk for sk in ResidentSpans(st, METRIC, START, END, engine=RecordingEngine()).span_keys
            if st.tagk.ids["dc"] in dict(sk[1]) and any(st.tagv.ids.get(f"h0{i}") == dict(sk[1]).get(st.tagk.ids["host"])
                                                          for i in range(10))]
    assert batch.n_series == len(want) > 0
    assert keys == sorted({(dict(sk[1])[st.tagk.ids["dc"]],) for sk in want})


# ---- ResidentSpans(device_tags=True) over a recording engine -------------------------------------
def test_resident_spans_device_tags():
    st = random_store(13)
    fe = RecordingEngine()
    rs = ResidentSpans(st, METRIC, START, END, engine=fe, device_tags=True)
    n = len(rs.span_keys)
    assert fe.calls == [("load", n), ("load_tags", n)]
    assert fe.table == [sorted(sk[1]) for sk in rs.span_keys]
    ptr, tk, tv = abi.tag_table_arrays(table_of(rs))
    assert ptr[0] == 0 and ptr[-1] == len(tk) == len(tv) and tk.dtype == tv.dtype == np.uint32 and ptr.dtype == np.int64
    for i in range(n):
        assert np.all(np.diff(tk[ptr[i]:ptr[i + 1]].astype(np.int64)) > 0)
    # the query goes as data; no host regroup
    q = query(st, {"dc": "*"}, [{"type": "not_literal_or", "tagk": "host", "filter": "h01"}])
    rs.run(q)
    assert fe.calls[-1][0] == "regroup_tags" and fe.calls[-1][1] == q.tag_query()
    assert not any(c[0] == "regroup" for c in fe.calls)
    # an unknown literal: nothing matches, no device query needed
    rs.run(query(st, {"dc": "nowhere"}))
    assert fe.calls[-1] == ("regroup", [abi.GROUP_EXCLUDED] * n)
    # an edit that adds a series reloads the table; one that adds none does not
    st.add_long(METRIC, START + 30, 5, {"host": "h00", "dc": "lga", "rack": "r0", "extra": "e"})
    before = len(fe.calls)
    rs.refresh(START, START + 3600)
    assert [c[0] for c in fe.calls[before:]] == ["upsert", "load_tags"] and fe.calls[-1] == ("load_tags", n + 1)
    assert fe.table == [sorted(sk[1]) for sk in rs.span_keys]
    before = len(fe.calls)
    rs.refresh(START, START + 3600)
    assert [c[0] for c in fe.calls[before:]] == ["upsert"]
    # a retire reloads it
    rs.spans[2] = (rs.spans[2][0], [])
    fe.new_index = np.asarray([i if i < 2 else (-1 if i == 2 else i - 1) for i in range(n + 1)])
    before = len(fe.calls)
    rs.retire_empty()
    assert [c[0] for c in fe.calls[before:]] == ["remove", "load_tags"] and fe.calls[-1] == ("load_tags", n)
    # the default keeps the host path: no table, a host regroup
    fe2 = RecordingEngine()
    rs2 = ResidentSpans(st, METRIC, START, END, engine=fe2)
    rs2.run(q)
    assert [c[0] for c in fe2.calls] == ["load", "regroup"]


# ---- plumbing -----------------------------------------------------------------------------------
def test_exports_option_header_sizes_and_symbols():
    for name in ("tsdbhip_tags_load", "tsdbhip_tags_loaded", "tsdbhip_regroup_tags", "tsdbhip_tags_keys"):
        assert name in engine.EXPORTS
    assert engine.OPTIONS.index("TAGS_SORT") == engine.OPTIONS.index("PUT_WALK") + 1 == engine.OPTIONS.index("TRACE") - 1
    hdr = open(os.path.join(ROOT, "include", "tsdbhip.h")).read()
    for text in ("int tsdbhip_tags_load(tsdbhip_ctx* ctx, const tsdbhip_tag_table* table);",
                 "int tsdbhip_tags_loaded(tsdbhip_ctx* ctx, int64_t* n_series, int64_t* n_tags);",
                 "enum { TSDB_TF_ANY = 0, TSDB_TF_IN, TSDB_TF_NOT_IN, TSDB_TF_NOT_KEY };", "#define TSDB_TAGS_DRY 1u",
                 "int tsdbhip_regroup_tags(tsdbhip_ctx* ctx, const tsdbhip_tag_query* query, uint32_t flags,",
                 "int tsdbhip_tags_keys(tsdbhip_ctx* ctx, uint32_t* keys);", "TAGS_SORT (1:", "#define TSDBHIP_ABI_VERSION 12"):
        assert text in hdr, text
    opts = open(os.path.join(ROOT, "opentsdb_amd", "csrc", "opts.h")).read()
    assert opts.index("OPT_PUT_WALK") < opts.index("OPT_TAGS_SORT") < opts.index("OPT_TRACE")
    assert (C.sizeof(abi.TagTable), C.sizeof(abi.TagFilter), C.sizeof(abi.TagQuery), C.sizeof(abi.TagsInfo)) == (32, 24, 56, 56)
    assert (abi.TF_ANY, abi.TF_IN, abi.TF_NOT_IN, abi.TF_NOT_KEY) == (TR.ANY, TR.IN, TR.NOT_IN, TR.NOT_KEY) == (0, 1, 2, 3)
    lib = engine.lib()
    assert lib.tsdbhip_abi_version() == 12
    q = abi.HostTagQuery([(1, abi.TF_IN, [2, 3])], [1])
    assert lib.tsdbhip_tags_load(None, None) == abi.TSDB_E_ILLEGAL_ARGUMENT
    assert lib.tsdbhip_tags_loaded(None, None, None) == abi.TSDB_E_ILLEGAL_ARGUMENT
    assert lib.tsdbhip_regroup_tags(None, C.byref(q.c), 0, None, None) == abi.TSDB_E_ILLEGAL_ARGUMENT
    assert lib.tsdbhip_tags_keys(None, None) == abi.TSDB_E_ILLEGAL_ARGUMENT
    engine.set_option("TAGS_SORT", 1)
    try:
        assert engine.get_option("TAGS_SORT") == 1
    finally:
        engine.set_option("TAGS_SORT", -1)
    assert engine.get_option("TAGS_SORT") == -1
