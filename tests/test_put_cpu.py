"""tsdbhip_put without a device: the expectation tests/put_util.py::put_batch -- the store's encoders
and the oracle's CompactionQueue over [(resident cell)] + the puts -- against MockStores built
from the full point lists, under both fix_duplicates settings, for every placement
tests/test_gpu_put.py runs on the device; the encodings at the length edges; the exports, the
option, the header text and the library's symbol (these fail without the feature).

A case is (series_points, gids, puts): series_points[i] the (timestamp, kind, value) writes that
make resident series i, puts the (series_index, timestamp, kind, value) writes of one call."""
from __future__ import annotations

import ctypes as C
import os
import struct

import numpy as np
import pytest

from opentsdb_amd import abi, engine, store
from tests.append_util import batches_equal, rows_of
from tests.put_util import D, F, L, bucket, encode, put_batch, store_batch, store_rows

T0 = 1356998400
H = 3600
EXCL = abi.GROUP_EXCLUDED
ILLEGAL_DATA = abi.TSDB_E_ILLEGAL_DATA
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def resident_row(n, base=T0):
    """n one-byte integers in one hour: every 20 s from offset 10 (n <= 129), or every second."""
    if n == 3600:
        return [(base + i, L, i % 100) for i in range(n)]
    assert n <= 129
    return [(base + 10 + 20 * i, L, (i * 7) % 100) for i in range(n)]


FIVE = [(T0 + o, L, v) for o, v in ((100, 1), (200, 2), (300, 3), (400, 4), (500, 5))]


def multi_case():
    rng = np.random.default_rng(5)
    series = [[(T0 + h * H + 30 + 60 * i, L, int(rng.integers(-100, 30000))) for h in range(3) for i in range(40)] for _ in range(5)]
    puts = []
    for s in range(5):
        for h in range(3):
            for k in range(1 + (s + h) % 3):
                puts.append((s, T0 + h * H + 45 + 60 * int(rng.integers(0, 59)), L, int(rng.integers(-100, 30000))))
    puts = [puts[i] for i in rng.permutation(len(puts))]
    # (two draws may share a second: both are 1-2-4-byte longs, so fix decides; keep distinct instants)
    seen, out = set(), []
    for p in puts:
        if (p[0], p[1]) not in seen:
            seen.add((p[0], p[1]))
            out.append(p)
    return series, [0, 1, 0, 1, 2], out


# name -> (series_points, gids, puts)
PLACEMENTS = {
    "before_first": ([FIVE], [0], [(0, T0 + 50, L, 9)]),
    "between": ([FIVE], [0], [(0, T0 + 250, L, 9)]),
    "after_last": ([FIVE], [0], [(0, T0 + 600, L, 9)]),
    "equal_same_bytes": ([FIVE], [0], [(0, T0 + 300, L, 3)]),
    "equal_other_bytes": ([FIVE], [0], [(0, T0 + 300, L, 300)]),          # a 2-byte long: another qualifier
    "second_and_ms_same_instant": ([FIVE], [0], [(0, T0 + 250, L, 9), (0, (T0 + 250) * 1000, L, 9)]),
    "second_and_ms_same_instant_other_bytes": ([FIVE], [0], [(0, T0 + 250, L, 9), (0, (T0 + 250) * 1000, L, 10)]),
    "ms_into_seconds_row": ([FIVE], [0], [(0, (T0 + 250) * 1000 + 500, L, 9), (0, (T0 + 700) * 1000 + 1, L, 7)]),
    "last_offsets": ([FIVE], [0], [(0, T0 + 3599, L, 9), (0, (T0 + 3599) * 1000 + 999, L, 8)]),
    "new_hours": ([[(T0 + H + 60 * i, L, i) for i in range(30)] + [(T0 + 3 * H + 60 * i, L, i) for i in range(30)]], [0],
                  [(0, T0 + 5, L, 1), (0, T0 + 2 * H + 5, L, 2), (0, T0 + 2 * H + 65, L, 3), (0, T0 + 4 * H + 5, L, 4)]),
    "zero_row_and_excluded": ([FIVE, [], FIVE], [0, 1, EXCL], [(1, T0 + 7, L, 1), (1, T0 + 67, L, 2), (2, T0 + 250, L, 3), (2, T0 + H + 5, L, 4)]),
    "same_qualifier_twice": ([FIVE], [0], [(0, T0 + 250, L, 1), (0, T0 + 260, L, 5), (0, T0 + 250, L, 2)]),
    "several_rows_of_several_series": multi_case(),
}
# the documented deviation: the put's qualifier already sits inside the resident cell
SAME_QUALIFIER_IN_CELL = ([FIVE], [0], [(0, T0 + 300, L, 77)])

LONG_EDGES = [-129, -128, 127, 128, -32768, 32768, 32767, -32769, (1 << 31) - 1, 1 << 31, -(1 << 31), -(1 << 31) - 1, -(1 << 63), (1 << 63) - 1]


def size_case(n, k, where):
    """A resident row of n datapoints and k puts: spread over the gaps (one before the first and
    one after the last where the row leaves room), or all behind the last."""
    rng = np.random.default_rng(1000 * n + 10 * k + len(where))
    res = resident_row(n)
    if n == 3600:   # every second is taken: the puts are millisecond points
        if where == "tail":
            offs = 3_599_000 + 1 + np.sort(rng.choice(998, k, replace=False))
        else:
            offs = np.sort(rng.choice(3599, k, replace=False)) * 1000 + 500   # (before the last second: never a tail)
        return [res], [0], [(0, T0 * 1000 + int(o), L, int(rng.integers(0, 100))) for o in rng.permutation(offs)]
    taken = {t - T0 for t, _, _ in res}
    last = max(taken)
    free = [o for o in range(3600) if o not in taken and (where != "tail" or o > last)]
    offs = set(int(o) for o in rng.choice(free, k, replace=False))
    if where != "tail":   # (one before the first datapoint, so that no draw is a tail; one after the last)
        offs = set(sorted(offs)[1:-1]) | ({5, 3590} if k >= 2 else {5})
    return [res], [0], [(0, T0 + int(o), L, int(rng.integers(0, 100))) for o in rng.permutation(sorted(offs))]


def full_store(series_points, gids, puts, fix):
    return store_batch([list(p) + [(ts, kind, v) for s, ts, kind, v in puts if s == i] for i, p in enumerate(series_points)], gids, fix)


def agree(case, fix):
    series_points, gids, puts = case
    a = store_batch(series_points, gids)
    got = put_batch(a, puts, fix)
    try:
        want = full_store(series_points, gids, puts, fix)
    except store.IllegalDataException:
        assert got == ILLEGAL_DATA
        return got
    assert not isinstance(got, int), got
    batches_equal(got.batch, want)
    return got


@pytest.mark.parametrize("fix", [False, True], ids=["nofix", "fix"])
@pytest.mark.parametrize("name", list(PLACEMENTS))
def test_put_batch_equals_the_full_store(name, fix):
    got = agree(PLACEMENTS[name], fix)
    if name in ("equal_other_bytes", "second_and_ms_same_instant_other_bytes"):
        assert (got == ILLEGAL_DATA) == (not fix)
    else:
        assert not isinstance(got, int)
    if name == "same_qualifier_twice":
        assert got.shadowed == 1 and bytes(got.batch.val[:7]) == bytes([1, 2, 2, 5, 3, 4, 5])
    if name == "new_hours":
        assert (got.added, got.rewritten) == (3, 0) and got.batch.n_rows == 5
    if name == "ms_into_seconds_row":
        assert got.batch.val[int(got.batch.row_val_off[1]) - 1] == store.MS_MIXED_COMPACT


@pytest.mark.parametrize("fix", [False, True], ids=["nofix", "fix"])
@pytest.mark.parametrize("where", ["spread", "tail"])
@pytest.mark.parametrize("k", [1, 2, 64, 65])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 3600])
def test_sizes_and_counts(n, k, where, fix):
    got = agree(size_case(n, k, where), fix)
    assert (got.added, got.rewritten, got.shadowed) == (0, 1, 0)


def test_the_compacted_column_deviation():
    """A put whose qualifier already sits inside the resident cell: the store's put overwrites
    that cell version, the engine's resident row is one compacted column and the put another.
    With fix_duplicates both keep the put; without it the store reads the put's value and the
    expectation (and tsdbhip_put) is an IllegalDataException."""
    series_points, gids, puts = SAME_QUALIFIER_IN_CELL
    a = store_batch(series_points, gids)
    assert put_batch(a, puts, False) == ILLEGAL_DATA
    want = full_store(series_points, gids, puts, False)
    assert bytes(want.val[:6]) == bytes([1, 2, 77, 4, 5, 0])
    batches_equal(put_batch(a, puts, True).batch, full_store(series_points, gids, puts, True))
    batches_equal(put_batch(a, puts, True).batch, want)


def test_single_datapoint_fixup_by_hand():
    """A resident single-datapoint row holding an 8-byte float under flags 0xB, plus one put:
    ColumnDatapointIterator drops the four leading zero bytes before the merge."""
    from opentsdb_amd import synth
    q = struct.pack(">H", (100 << 4) | 0xB)
    a = synth.from_series([[(T0, q, b"\x00\x00\x00\x00" + struct.pack(">f", 1.5))]], [0])
    got = put_batch(a, [(0, T0 + 200, F, 2.5)], False)
    (base, mq, mv), = rows_of(got.batch, 0)
    assert mq == q + struct.pack(">H", (200 << 4) | 0xB)
    assert mv == struct.pack(">f", 1.5) + struct.pack(">f", 2.5) + b"\x00"
    # the put at the fixed datapoint's own offset wins; its bytes are compared with the fixed value's
    assert put_batch(a, [(0, T0 + 100, F, 1.5)], False).batch.val.tobytes() == struct.pack(">f", 1.5)
    assert put_batch(a, [(0, T0 + 100, F, 2.5)], False) == ILLEGAL_DATA
    bad = synth.from_series([[(T0, q, b"\x00\x00\x00\x01" + struct.pack(">f", 1.5))]], [0])
    assert put_batch(bad, [(0, T0 + 200, F, 2.5)], False) == ILLEGAL_DATA


def test_encodings_at_the_length_edges():
    want = {-129: 2, -128: 1, 127: 1, 128: 2, -32768: 2, 32768: 4, 32767: 2, -32769: 4, (1 << 31) - 1: 4, 1 << 31: 8,
            -(1 << 31): 4, -(1 << 31) - 1: 8, -(1 << 63): 8, (1 << 63) - 1: 8}
    assert set(want) == set(LONG_EDGES)
    for v, n in want.items():
        base, q, b = encode(T0 + 7, L, v)
        assert (base, len(b), q) == (T0, n, struct.pack(">H", (7 << 4) | (n - 1))), v
        assert int.from_bytes(b, "big", signed=True) == v
        assert abi.point_bits(L, v) == v & 0xFFFFFFFFFFFFFFFF
    base, q, b = encode((T0 + 3599) * 1000 + 999, F, 0.25)
    assert (base, q, b) == (T0, struct.pack(">I", 0xF0000000 | (3599999 << 6) | 0xB), struct.pack(">f", 0.25))
    base, q, b = encode(T0 + 3599, D, 0.1)
    assert (q, b) == (struct.pack(">H", (3599 << 4) | 0xF), struct.pack(">d", 0.1))
    assert abi.point_bits(F, 0.25) == 0x3E800000 and abi.point_bits(D, -0.0) == 1 << 63
    rows, shadowed = bucket([(0, T0 + 1, L, 1), (0, T0 + 1, L, 2), (0, T0 + 1, L, 300), (1, T0 + 1, L, 1)])
    assert shadowed == 1 and [v for _, v in rows[(0, T0)]] == [b"\x02", b"\x01\x2c"]
    pts = abi.make_points([(3, T0 + 1, L, -1), (4, (T0 + 1) * 1000, D, 1.0)])
    assert pts.dtype.itemsize == C.sizeof(abi.Point) == 32 and pts["bits"][0] == 0xFFFFFFFFFFFFFFFF
    assert (abi.PUT_LONG, abi.PUT_FLOAT, abi.PUT_DOUBLE, abi.PUT_FIX_DUPLICATES) == (1, 2, 3, 1)


# ---- ResidentSpans.put ---------------------------------------------------------------------------
class PutEngine:
    """Records what ResidentSpans hands the engine."""

    def __init__(self, refuse=False):
        self.puts, self.upserts, self.refuse = [], [], refuse

    def load(self, batch):
        self.loaded = batch

    def put(self, points, fix_duplicates=False):
        self.puts.append((list(points), fix_duplicates))
        if self.refuse:
            raise engine.EngineError(self.refuse, "refused")
        return abi.PutInfo()

    def upsert(self, delta, series_index, series_new):
        self.upserts.append((delta, list(series_index), list(series_new)))
        return abi.UpsertInfo()


def spans_store(fix=False):
    st = store.MockStore(fix_duplicates=fix)
    for h in ("a", "b"):
        for i in range(10):
            st.add_long("m", T0 + 60 * i, i, {"host": h})
            st.add_long("m", T0 + H + 60 * i, i, {"host": h})
    return st


@pytest.mark.parametrize("refuse", [0, ILLEGAL_DATA, abi.TSDB_E_NOT_IMPLEMENTED], ids=["put", "illegal_data", "not_implemented"])
def test_resident_spans_put_and_its_fallback(refuse):
    from opentsdb_amd.query import ResidentSpans
    st = spans_store(fix=True)
    fe = PutEngine(refuse)
    rs = ResidentSpans(st, "m", T0, T0 + 2 * H, engine=fe)
    pts = [({"host": "a"}, T0 + 30, L, 7), ({"host": "b"}, (T0 + H + 45) * 1000, D, 0.5), ({"host": "c"}, T0 + H + 5, L, 1),
           ({"host": "a"}, T0 + 5 * H, L, 9)]
    info, ups = rs.put(pts)
    (sent, fixd), = fe.puts
    assert fixd is True and sent == [(0, T0 + 30, L, 7), (1, (T0 + H + 45) * 1000, D, 0.5)]
    # host c is new (its hour is rescanned), the point outside the range only reaches the store
    hours = [sorted(set(d.row_base_time.tolist())) for d, _, _ in fe.upserts]
    assert hours == ([[T0], [T0 + H]] if refuse else [[T0 + H]]) and len(ups) == len(hours)
    assert (info is None) == bool(refuse)
    if refuse:   # any other refusal is the caller's to see
        fe.refuse = abi.TSDB_E_ILLEGAL_ARGUMENT
        with pytest.raises(engine.EngineError):
            rs.put([({"host": "a"}, T0 + 31, L, 7)])
        return
    fresh = ResidentSpans(st, "m", T0, T0 + 2 * H, engine=PutEngine())
    assert rs.span_keys == fresh.span_keys and rs.spans == fresh.spans
    assert (st.metrics.ids["m"], st._series_uids("m", {"host": "a"})[1], T0 + 5 * H) in st.rows


# ---- the C entry point without a device ----------------------------------------------------------
def test_exports_option_header_and_symbol():
    assert "tsdbhip_put" in engine.EXPORTS and "PUT_WALK" in engine.OPTIONS
    assert engine.OPTIONS.index("PUT_WALK") == engine.OPTIONS.index("LAST_WALK") + 1
    hdr = open(os.path.join(ROOT, "include", "tsdbhip.h")).read()
    for text in ("int tsdbhip_put(tsdbhip_ctx* ctx, const tsdbhip_point* pts, int64_t n, uint32_t flags, tsdbhip_put_info* info",
                 "TSDB_PUT_LONG = 1, TSDB_PUT_FLOAT = 2, TSDB_PUT_DOUBLE = 3", "#define TSDB_PUT_FIX_DUPLICATES 1u",
                 "PUT_WALK (1:", "#define TSDBHIP_ABI_VERSION 12"):
        assert text in hdr, text
    opts = open(os.path.join(ROOT, "opentsdb_amd", "csrc", "opts.h")).read()
    assert opts.index("OPT_LAST_WALK") < opts.index("OPT_PUT_WALK") < opts.index("OPT_TRACE")
    lib = engine.lib()
    assert lib.tsdbhip_put(None, None, 0, 0, None) == abi.TSDB_E_ILLEGAL_ARGUMENT
    pts = abi.make_points([(0, T0, L, 1)])
    info = abi.PutInfo()
    assert lib.tsdbhip_put(None, pts.ctypes.data, 1, 0, C.byref(info)) == abi.TSDB_E_ILLEGAL_ARGUMENT
    assert C.sizeof(abi.PutInfo) == 96 and lib.tsdbhip_abi_version() == 12
    engine.set_option("PUT_WALK", 1)
    try:
        assert engine.get_option("PUT_WALK") == 1
    finally:
        engine.set_option("PUT_WALK", -1)
