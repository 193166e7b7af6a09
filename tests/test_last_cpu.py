"""Host side of the last-datapoint query (tsdbhip_last, Engine.last, query.ResidentSpans.last): the
plain-Python reference tests/last_ref.py against the reference's own known answers and against the
oracle's raw `none` query, the argument checks that need no device, abi.LastInfo against the
header, and ResidentSpans.last's sub-query logic over a stub engine."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import pytest

from opentsdb_amd import abi, engine, synth
from opentsdb_amd.query import LastPoint, ResidentSpans
from opentsdb_amd.store import MockStore
from oracle import oracle as O
from tests import last_ref as R
from tests.test_regroup_cpu import END, METRIC, START, TAGS, FakeEngine, make_store
from tests.test_remove_cpu import header_fields

T0 = 1356998400
H = 3600
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "last_point.json")


def golden_cases():
    return json.load(open(GOLDEN))["cases"]


# ---- last_ref against the reference's own tests ---------------------------------------------------
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"].split()[0])
def test_last_ref_reproduces_the_reference_tests(case):
    st = MockStore()
    for ts, v in case["points"]:
        st.add_long("sys.cpu.user", ts, v, {"host": "web01"})
    spans = st.scan("sys.cpu.user", 0, 1 << 32)
    batch = synth.from_series([rows for _, rows in spans], [0] * len(spans))
    if case["expect"] == "IllegalArgumentException":
        with pytest.raises(ValueError):
            R.last_ref(batch, None, case["now_s"], None, case["back_scan"])
        return
    ts, bits, kind = R.last_ref(batch, None, case["now_s"], None, case["back_scan"])
    if case["expect"] is None:
        assert (int(ts[0]), int(bits[0]), int(kind[0])) == (0, 0, R.KIND_NONE)
    else:
        assert (int(ts[0]), int(bits[0]), int(kind[0])) == (case["expect"][0], case["expect"][1], R.KIND_INT)


def test_the_literal_hour_loop_ends_for_any_back_scan():
    rows = {T0: (b"\x00\x00", b"\x07")}
    assert R.last_point(rows, T0 + 10 ** 6 * H + 5, 2 ** 31 - 1) == (T0 * 1000, R.KIND_INT, 7)
    assert R.last_point(rows, T0 - 1, 2 ** 31 - 1) is None
    assert R.last_point({}, T0, 2 ** 31 - 1) is None


# ---- last_ref against the oracle's decoder --------------------------------------------------------
def sorted_store():
    """Series of every value type and qualifier width over three hours, irregular spacing, no two
    alike: what TSDB.addPoint and the compaction write (sorted cells)."""
    rng = np.random.default_rng(11)
    series = []
    for s in range(14):
        n = int(rng.integers(1, 200))
        ts = np.sort(rng.choice(3 * H * 1000, n, replace=False)) + T0 * 1000
        ms = np.zeros(n, bool) if s % 3 == 0 else np.ones(n, bool) if s % 3 == 1 else rng.random(n) < 0.5
        ts = np.where(ms, ts, ts // 1000 * 1000)
        keep = np.concatenate([[True], np.diff(ts) > 0])
        ts, ms = ts[keep], ms[keep]
        kind = np.full(len(ts), s % 3 if s < 9 else 0) if s < 12 else rng.integers(0, 3, len(ts))
        lv = rng.integers(-(1 << 62), 1 << 62, len(ts)) >> rng.integers(0, 62, len(ts))
        fv = rng.standard_normal(len(ts)) * 1e3
        series.append(synth.encode_rows(ts, lv, fv, kind, ms))
    return synth.from_series(series, list(range(len(series))))


def test_last_ref_equals_the_last_point_of_the_oracles_raw_none_query():
    b = sorted_store()
    out = O.run_query(b, abi.new_query(T0, T0 + 3 * H, "none"))
    assert len(out) == b.n_series
    last_base = [int(b.row_base_time[int(b.series_row_ptr[s + 1]) - 1]) for s in range(b.n_series)]
    ts, bits, kind = R.last_ref(b, None, 0, [x + 1234 for x in last_base], 0)
    for s, (_, ots, obits, oint) in enumerate(out):
        assert int(ts[s]) == int(ots[-1])
        assert int(kind[s]) == (R.KIND_INT if oint[-1] else R.KIND_FLOAT)
        assert int(bits[s]) == int(np.asarray(obits).view(np.uint64)[-1])
    # and one anchor for all, looking back from the store's last hour
    ts2, bits2, kind2 = R.last_ref(b, None, T0 + 3 * H - 1, None, 2)
    assert np.array_equal(ts, ts2) and np.array_equal(bits, bits2) and np.array_equal(kind, kind2)


def test_ties_take_the_later_cell_and_unsorted_cells_their_maximum():
    q = (R.H - 1 << 4).to_bytes(2, "big") + (5 << 4).to_bytes(2, "big") + (R.H - 1 << 4).to_bytes(2, "big")
    assert R.last_of_row(T0, q, b"\x01\x02\x03\x00") == ((T0 + H - 1) * 1000, R.KIND_INT, 3)
    q = (9 << 4 | 0xB).to_bytes(2, "big") + (5 << 4).to_bytes(2, "big")
    assert R.last_of_row(T0, q, b"\x3f\xc0\x00\x00\xff\x00") == ((T0 + 9) * 1000, R.KIND_FLOAT, 0x3FF8000000000000)
    assert R.last_of_row(T0, (7 << 4 | 7).to_bytes(2, "big"), b"\x80" + b"\x00" * 7) == ((T0 + 7) * 1000, R.KIND_INT, 1 << 63)
    with pytest.raises(R.IllegalData):
        R.last_of_row(T0, b"\x00\x01\x00\xa1", b"\x00\x01\x02")


# ---- the C entry point without a device -----------------------------------------------------------
def test_export_and_illegal_arguments_need_no_device():
    assert "tsdbhip_last" in engine.EXPORTS and "LAST_WALK" in engine.OPTIONS
    L = engine.lib()
    IA = abi.TSDB_E_ILLEGAL_ARGUMENT
    ts, bits, kind = np.zeros(4, np.int64), np.zeros(4, np.uint64), np.zeros(4, np.uint8)
    sel = np.zeros(4, np.int64)
    info = abi.LastInfo()
    args = (ts.ctypes.data, bits.ctypes.data, kind.ctypes.data, C.byref(info))
    assert L.tsdbhip_last(None, sel.ctypes.data, 4, T0, None, 0, *args) == IA            # null context
    assert L.tsdbhip_last(None, None, 0, T0, None, 0, None, None, None, None) == IA
    assert L.tsdbhip_last(None, sel.ctypes.data, -1, T0, None, 0, *args) == IA
    assert L.tsdbhip_last(None, sel.ctypes.data, 4, T0, None, -1, *args) == IA
    assert L.tsdbhip_last(None, sel.ctypes.data, 4, -1, None, 0, *args) == IA
    assert L.tsdbhip_abi_version() == 12
    assert (abi.LAST_NONE, abi.LAST_INT, abi.LAST_FLOAT) == (R.KIND_NONE, R.KIND_INT, R.KIND_FLOAT)


def test_last_info_matches_the_header():
    hdr = open(os.path.join(os.path.dirname(engine.HERE), "include", "tsdbhip.h")).read()
    import re
    body = re.search(r"typedef struct \{([^}]*)\} tsdbhip_last_info;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    ctypes_of = {"int64_t": C.c_int64, "double": C.c_double}
    for decl in body.split(";"):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctypes_of[ctype]) for n in names.split(",")]
    assert fields == list(abi.LastInfo._fields_)
    assert C.sizeof(abi.LastInfo) == 48
    assert [getattr(abi.LastInfo, n).offset for n, _ in fields] == [0, 8, 16, 24, 32, 40]
    assert header_fields(hdr, "tsdbhip_remove_range") == list(abi.RemoveRange._fields_)   # (the shared parser still reads the header)
    assert "#define TSDBHIP_ABI_VERSION 12" in hdr


# ---- ResidentSpans.last over a stub engine --------------------------------------------------------
class LastEngine(FakeEngine):
    """Records the last() calls and answers them with last_ref over the loaded batch."""

    def __init__(self):
        super().__init__()
        self.lasts = []

    def last(self, series_index=None, anchor_s=0, anchor_each=None, back_scan=0):
        self.lasts.append((None if series_index is None else list(series_index), anchor_s,
                           None if anchor_each is None else list(anchor_each), back_scan))
        ts, bits, kind = R.last_ref(self.loaded, series_index, anchor_s, anchor_each, back_scan)
        return ts, bits, kind, abi.LastInfo()


@pytest.fixture(scope="module")
def resident():
    st = make_store()
    fe = LastEngine()
    return st, fe, ResidentSpans(st, METRIC, START, END, engine=fe)


def tsuid(st, tags):
    m = st.metrics.ids[METRIC]
    t = sorted((st.tagk.ids[k], st.tagv.ids[v]) for k, v in tags.items())
    return (m.to_bytes(3, "big") + b"".join(k.to_bytes(3, "big") + v.to_bytes(3, "big") for k, v in t)).hex().upper()


def expected(st, tags, now_s, back_scan):
    """The answer from the store itself: the last point of the newest row inside the window."""
    spans = dict(st.scan(METRIC, START, END))
    key = (st.metrics.ids[METRIC], tuple(sorted((st.tagk.ids[k], st.tagv.ids[v]) for k, v in tags.items())))
    got = R.last_point({b: (q, v) for b, q, v in spans.get(key, [])}, now_s, back_scan)
    if got is None:
        return None
    return got[0], float(np.uint64(got[2]).view(np.float64))


def test_sub_queries_by_tsuid_and_by_metric_and_tags(resident):
    st, fe, rs = resident
    fe.lasts.clear()
    now = END - 1
    subs = [{"tsuids": [tsuid(st, TAGS[3]), "00000100000A00000B", tsuid(st, TAGS[0]).lower()], "metric": "ignored.when.tsuids.are.given"},
            {"metric": METRIC, "tags": TAGS[5]},
            {"metric": METRIC, "tags": {"host": "web01", "dc": "ams"}},      # known names, no such series
            {"metric": METRIC, "tags": {"host": "nobody"}},                  # an unknown tag value
            {"metric": METRIC, "tags": TAGS[4]}]                             # rows in the first hour only: none at back_scan 0
    out = rs.last(subs, back_scan=0, now_s=now)
    assert all(isinstance(p, LastPoint) for p in out)
    assert [p.tsuid for p in out] == [tsuid(st, TAGS[3]), tsuid(st, TAGS[0]), tsuid(st, TAGS[5])]
    for p, tags in zip(out, (TAGS[3], TAGS[0], TAGS[5])):
        assert (p.timestamp, p.value) == expected(st, tags, now, 0) and isinstance(p.value, float)
    (sel, anchor, each, bs), = fe.lasts                                      # one engine call for all of them
    keys = [rs.tsuid_of(sk) for sk in rs.span_keys]
    assert sel == [keys.index(tsuid(st, t)) for t in (TAGS[3], TAGS[0], TAGS[5], TAGS[4])]
    assert (anchor, each, bs) == (now, None, 0)
    # the back scan reaches the first hour of the series that stopped there
    out = rs.last([{"metric": METRIC, "tags": TAGS[4]}], back_scan=3, now_s=now)
    assert [(p.timestamp, p.value) for p in out] == [expected(st, TAGS[4], now, 3)] and expected(st, TAGS[4], now, 2) is None
    assert rs.last([{"metric": METRIC, "tags": TAGS[4]}], back_scan=2, now_s=now) == []


def test_last_write_times_anchor_each_series_only_without_a_back_scan(resident):
    st, fe, rs = resident
    fe.lasts.clear()
    a, b, c = tsuid(st, TAGS[4]), tsuid(st, TAGS[0]), tsuid(st, TAGS[1])
    writes = {a: START + 17, b.lower(): START + 2 * H + 5}                   # (c has no counter in the meta table)
    out = rs.last([{"tsuids": [a, b, c]}], back_scan=0, now_s=END - 1, last_write_s=writes)
    assert [p.tsuid for p in out] == [a, b]
    assert (out[0].timestamp, out[0].value) == expected(st, TAGS[4], START + 17, 0)
    assert (out[1].timestamp, out[1].value) == expected(st, TAGS[0], START + 2 * H + 5, 0)
    assert fe.lasts[-1][2] == [START + 17, START + 2 * H + 5] and fe.lasts[-1][3] == 0
    out = rs.last([{"tsuids": [a, b, c]}], back_scan=4, now_s=END - 1, last_write_s=writes)
    assert [p.tsuid for p in out] == [a, b, c] and fe.lasts[-1][1:] == (END - 1, None, 4)


def test_refusals_and_empty_answers(resident):
    st, fe, rs = resident
    fe.lasts.clear()
    with pytest.raises(ValueError, match="another metric"):
        rs.last([{"metric": "sys.cpu.system", "tags": TAGS[0]}], now_s=END - 1)
    with pytest.raises(ValueError, match="Backscan"):
        rs.last([{"tsuids": [tsuid(st, TAGS[0])]}], back_scan=-1, now_s=END - 1)
    assert rs.last([], now_s=END - 1) == [] and rs.last([{"tsuids": ["FFFFFF"]}], now_s=END - 1) == []
    assert fe.lasts == []                                                    # nothing to ask: no engine call


def test_integer_values_come_back_as_python_ints():
    st = MockStore()
    st.add_long(METRIC, T0 + 5, -(1 << 63), {"host": "a"})
    st.add_long(METRIC, T0 + 9, -129, {"host": "b"})
    fe = LastEngine()
    rs = ResidentSpans(st, METRIC, T0, T0 + H, engine=fe)
    out = rs.last([{"metric": METRIC, "tags": {"host": "a"}}, {"metric": METRIC, "tags": {"host": "b"}}], now_s=T0 + 100)
    assert [(p.timestamp, p.value) for p in out] == [((T0 + 5) * 1000, -(1 << 63)), ((T0 + 9) * 1000, -129)]
    assert all(type(p.value) is int for p in out)
