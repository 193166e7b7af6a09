"""GPU parity of tsdbhip_last (k_last.hip): the newest datapoint of each selected resident series.

The expectation never comes from the engine.  Every case compares ts_ms, bits and kind array for
array with tests/last_ref.py (the reference's hour loop and cell sort, restated in plain Python and
checked against the reference's own tests and the oracle in tests/test_last_cpu.py), and
info.direct / copied / walked / none with counts predicted on the host from tests/index_ref.py's row
facts and the route rules of DESIGN.md 5.16:

    direct  not ROW_UNSORTED, one qualifier width, a uniform value length
    copied  not ROW_UNSORTED, 2-byte qualifiers, varying lengths, ROW_VLE2 and ROW_ALLI, the int16 copy
            present (it is whenever a resident row of 2-byte qualifiers and 1-2-byte integers exists)
    walked  everything else

Every case then repeats under LAST_WALK=1: the same answers, all of them walked."""
from __future__ import annotations

import os
import re
import struct
from functools import lru_cache

import numpy as np
import pytest

from opentsdb_amd import abi, synth
from opentsdb_amd import engine as E
from tests import index_ref as IX
from tests import last_ref as R
from tests.append_util import Points, int_points, merge_batches, quarter_points, split
from tests.index_ref import q2, q4
from tests.remove_util import remove_batch
from tests.test_gpu_regroup import dsq, identical
from tests.trim_util import trim_batch

gpu = pytest.mark.gpu

T0 = 1356998400
H = 3600
INT32_MAX = 2 ** 31 - 1
EXCL, NONE = abi.GROUP_EXCLUDED, abi.GROUP_NONE
NO_PACK = abi.TRIM_NO_PACK


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def walk_grid_waves():
    """k_last_walk's grid cap in waves, read from the kernel file's named constants."""
    src = open(os.path.join(E.CSRC, "k_last.hip")).read()
    block = int(re.search(r"constexpr int LAST_BLOCK = (\d+);", src).group(1))
    blocks = int(re.search(r"constexpr int64_t LAST_WALK_MAX_BLOCKS = (\d+);", src).group(1))
    return blocks * (block // 64)


# ---- the expectation ------------------------------------------------------------------------------
_facts = {}


def row_flags(batch):
    """index_ref's flags of every row, computed once a batch."""
    if id(batch) not in _facts:
        _facts[id(batch)] = (batch, IX.index_ref(batch)[1])
    return _facts[id(batch)][1]


def predict(batch, sel, anchor_s, anchor_each, back_scan):
    """(direct, copied, walked, none) of the call, or None when an answer row is malformed."""
    flags = row_flags(batch)
    srp = batch.series_row_ptr
    copy = any((int(f) & (IX.ROW_QW_MASK | IX.ROW_ALLI | IX.ROW_VLE2 | IX.ROW_ERR)) == (2 | IX.ROW_ALLI | IX.ROW_VLE2) for f in flags)
    n = [0, 0, 0, 0]
    for k, s in enumerate(range(batch.n_series) if sel is None else sel):
        rows = {int(batch.row_base_time[r]): r for r in range(int(srp[s]), int(srp[s + 1]))}
        h = R.answer_base(rows, int(anchor_each[k]) if anchor_each is not None else anchor_s, back_scan)
        if h is None:
            n[3] += 1
            continue
        f = int(flags[rows[h]])
        if f & IX.ROW_ERR:
            return None
        qw, vl = f & IX.ROW_QW_MASK, (f & IX.ROW_VL_MASK) >> IX.ROW_VL_SHIFT
        plain = not (f & IX.ROW_UNSORTED) and qw in (2, 4)
        if plain and vl:
            n[0] += 1
        elif plain and qw == 2 and (f & IX.ROW_VLE2) and (f & IX.ROW_ALLI) and copy:
            n[1] += 1
        else:
            n[2] += 1
    return tuple(n)


def check_last(eng, batch, sel=None, anchor_s=0, anchor_each=None, back_scan=0, ctx="", routes=None):
    """One call against last_ref over `batch` (what the context holds), as routed and under
    LAST_WALK=1.  routes: the (direct, copied, walked, none) the caller expects on top."""
    want = R.last_ref(batch, sel, anchor_s, anchor_each, back_scan)
    n = predict(batch, sel, anchor_s, anchor_each, back_scan)
    if routes is not None:
        assert n == tuple(routes), (ctx, n, routes)
    for walk in (None, 1):
        with E.options(LAST_WALK=walk):
            ts, bits, kind, info = eng.last(sel, anchor_s, anchor_each, back_scan)
        for name, g, w in zip(("ts_ms", "bits", "kind"), (ts, bits, kind), want):
            assert g.dtype == w.dtype
            np.testing.assert_array_equal(g, w, err_msg=f"{ctx} walk={walk}: {name}")
        got = (info.direct, info.copied, info.walked, info.none)
        assert got == (n if walk is None else (0, 0, n[0] + n[1] + n[2], n[3])), (ctx, walk, got, n)
        assert info.found == n[0] + n[1] + n[2] and info.found + info.none == len(ts) and info.kernel_ms >= 0.0
    return want


# ---- cell builders --------------------------------------------------------------------------------
LEN = {"i1": 1, "i2": 2, "i4": 4, "i8": 8, "f4": 4, "f8": 8}


def vbytes(typ, x):
    if typ == "f4":
        return np.array([x], ">f4").tobytes()
    if typ == "f8":
        return np.array([x], ">f8").tobytes()
    return int(x).to_bytes(LEN[typ], "big", signed=True)


def cell(points):
    """(qualifiers, values) of [(offset, in ms, type, value)] in the order given, as the compaction
    writes them: a meta byte after two or more values, MS_MIXED_COMPACT when the widths mix."""
    q, v = [], []
    for off, ms, typ, x in points:
        fl = (8 if typ[0] == "f" else 0) | (LEN[typ] - 1)
        q.append(q4(off, fl) if ms else q2(off, fl))
        v.append(vbytes(typ, x))
    meta = b"" if len(points) < 2 else (b"\x01" if len({p[1] for p in points}) == 2 else b"\x00")
    return b"".join(q), b"".join(v) + meta


def offsets(rng, n, ms, regular):
    """n ascending offsets ending at the hour's last second / millisecond."""
    top = H * 1000 - 1 if ms else H - 1
    if regular:
        step = max(1, min(top // max(1, n - 1), 7)) if n > 1 else 1
        return [top - (n - 1 - i) * step for i in range(n)]
    return sorted(int(x) for x in rng.choice(top, n - 1, replace=False)) + [top]


SPECIAL = {"i1": [-1, 127, -128], "i2": [-129, 32767, -32768], "i4": [-(1 << 31), (1 << 31) - 1, -32769],
           "i8": [-(1 << 63), (1 << 63) - 1, -1], "f4": [float("nan"), -0.0, float("inf"), float("-inf"), 1.5],
           "f8": [float("nan"), -0.0, float("inf"), float("-inf"), 0.1]}


@lru_cache(maxsize=None)
def direct_store():
    """One row a series: 1, 2, 64 and 65 datapoints x both qualifier widths x every value type x
    regular and irregular spacing, the last value a boundary of its type."""
    rng = np.random.default_rng(3)
    series = []
    turn = {typ: 0 for typ in LEN}
    for n in (1, 2, 64, 65):
        for ms in (False, True):
            for typ in LEN:
                for regular in (True, False):
                    offs = offsets(rng, n, ms, regular)
                    sp = SPECIAL[typ]
                    vals = [sp[(i + len(series)) % len(sp)] for i in range(n)]
                    vals[-1] = sp[turn[typ] % len(sp)]                         # every boundary value ends some row
                    turn[typ] += 1
                    series.append([(T0, *cell([(o, ms, typ, x) for o, x in zip(offs, vals)]))])
    return synth.from_series(series, [i % 5 for i in range(len(series))])


@lru_cache(maxsize=None)
def copied_store():
    """2-byte qualifiers, 1- and 2-byte integers with negative values; the last value of either
    length; one row of 1-byte values only (a uniform length: direct) and a float row beside them."""
    rng = np.random.default_rng(4)
    series = []
    for n in (2, 3, 64, 65, 300):
        for last in (-1, -129, 30000, 5):
            for regular in (True, False):
                offs = offsets(rng, n, False, regular)
                vals = [int(x) for x in rng.integers(-300, 300, n)]
                vals[0], vals[-1] = (-200 if abs(last) < 128 else 7), last      # both lengths in every row
                series.append([(T0, *cell([(o, False, "i1" if -128 <= x <= 127 else "i2", x) for o, x in zip(offs, vals)]))])
    series.append([(T0, *cell([(o, False, "i1", -5) for o in (0, 10, 20)]))])
    series.append([(T0, *cell([(o, False, "f4", 0.25) for o in (0, 10, 3599)]))])
    return synth.from_series(series, [0] * len(series))


def vle_row(rng, n, top=None):
    """n sorted datapoints of 2-byte qualifiers whose types vary: lengths 1 / 2 / 4 / 8 and floats."""
    offs = list(range(n)) if top is None else sorted(int(x) for x in rng.choice(top, n, replace=False))
    types = list(LEN)
    pts = []
    for i, o in enumerate(offs):
        typ = types[int(rng.integers(0, 6))] if i > 1 else ("i8", "i1")[i]   # (never one length throughout)
        x = float(rng.integers(-999, 999)) * 0.5 if typ[0] == "f" else int(rng.integers(-(1 << (8 * LEN[typ] - 1)), 1 << (8 * LEN[typ] - 1)))
        pts.append((o, False, typ, x))
    return pts


@lru_cache(maxsize=None)
def walked_store():
    rng = np.random.default_rng(5)
    series = []
    # mixed widths: ending in a 2-byte qualifier after 4-byte ones, and the reverse
    series.append([(T0, *cell([(1500, True, "i2", -300), (2750, True, "f4", 2.5), (3000, True, "i1", 9), (7, False, "i4", -70000)]))])
    series.append([(T0, *cell([(1, False, "i1", 1), (2, False, "f8", -0.0), (3, False, "i2", 400), (3599999, True, "i8", -(1 << 63))]))])
    series.append([(T0, *cell([(i, False, "i1", i) for i in range(70)] + [(70500 + i, True, "f4", i + 0.5) for i in range(70)]))])
    # varying lengths and types in rows of 63, 64, 65, 129 and 3600 datapoints
    for n in (63, 64, 65, 129, 3600):
        series.append([(T0, *cell(vle_row(rng, n)))])
    # cells unsorted in themselves: the maximum first, in the middle, on either side of a 64-datapoint step
    for n, at in ((130, 0), (130, 65), (130, 63), (130, 64), (130, 127), (130, 128), (5, 2)):
        pts = vle_row(rng, n, top=3000)
        o, ms, typ, x = pts[at]
        pts[at] = (3400, ms, "i2", -12345)
        series.append([(T0, *cell(pts))])
    # two equal maximal offsets with different values: the later one wins
    series.append([(T0, *cell([(10, False, "i1", 1), (3000, False, "i2", 1111), (20, False, "i1", 2), (3000, False, "f4", -2.25), (30, False, "i1", 3)]))])
    series.append([(T0, *cell([(3000, False, "i1", 1)] + [(i, False, "i1", 2) for i in range(100)] + [(3000, False, "i4", 99999)]))])
    # a row flagged only across rows: the first hour's last datapoint lies past the second hour's first
    series.append([(T0, *cell([(0, False, "f4", 1.0), (3700, False, "f4", 2.0)])), (T0 + H, *cell([(50, False, "f4", 3.0), (900, False, "f4", 4.0)]))])
    return synth.from_series(series, [i % 3 for i in range(len(series))])


def one_point(base, off, x):
    return (base, *cell([(off, False, "i2", x)]))


@lru_cache(maxsize=None)
def lookup_store():
    """Series of 0, 1, 2, 3, 24 and 25 one-point rows, consecutive hours and with gaps."""
    series = []
    for n in (0, 1, 2, 3, 24, 25):
        for gap in (1, 3):
            series.append([one_point(T0 + k * gap * H, (7 * k) % 3600, 100 * n + k) for k in range(n)])
    return synth.from_series(series, [0] * len(series))


def load(eng, batch, **opts):
    with E.options(**opts):
        eng.load(batch)
    return batch


# ---- routes ---------------------------------------------------------------------------------------
@gpu
def test_direct(eng):
    b = load(eng, direct_store())
    n = b.n_series
    assert n == 4 * 2 * 6 * 2
    want = check_last(eng, b, None, T0 + 1800, None, 0, "direct", routes=(n, 0, 0, 0))
    # what the store was built to end in: the hour's last second / millisecond, every boundary value
    assert set(want[0].tolist()) == {(T0 + H) * 1000 - 1000, (T0 + H) * 1000 - 1}
    seen = {(int(k), int(x)) for k, x in zip(want[2], want[1])}
    for x in (-1, -129, -(1 << 31), -(1 << 63)):
        assert (1, x & 0xFFFFFFFFFFFFFFFF) in seen
    for x in (float("nan"), -0.0, float("inf"), float("-inf")):
        assert (2, struct.unpack(">Q", struct.pack(">d", x))[0]) in seen
    _, flags, _, _, facts = IX.index_ref(b)
    assert all(f.ndp in (1, 2, 64, 65) for f in facts) and {f.qw for f in facts} == {2, 4}


@gpu
@pytest.mark.parametrize("opts", [{}, {"INDEX_FUSED": 0}, {"INDEX_GENERIC": 1}], ids=["fused", "classes_first", "generic"])
def test_copied(eng, opts):
    b = load(eng, copied_store(), **opts)
    n = b.n_series
    # the int16 copy exists on every index route (a 2-byte-qualifier row of 1-2-byte integers is resident)
    check_last(eng, b, None, T0, None, 0, f"copied {opts}", routes=(2, n - 2, 0, 0))


@gpu
def test_rows_of_varying_lengths_walk_without_small_integers(eng):
    """Varying lengths beyond 2 bytes: no copy can hold the values, the rows walk."""
    rng = np.random.default_rng(6)
    b = load(eng, synth.from_series([[(T0, *cell(vle_row(rng, n)))] for n in (2, 64, 65)], [0, 0, 0]))
    check_last(eng, b, None, T0 + 5, None, 0, "vle", routes=(0, 0, 3, 0))


@gpu
def test_walked(eng):
    b = load(eng, walked_store())
    n = b.n_series
    want = check_last(eng, b, None, T0 + 100, None, 0, "walked", routes=(1, 0, n - 1, 0))   # (the last series' first hour is plain)
    ts, bits, kind = (x.tolist() for x in want)
    assert (ts[0], kind[0], bits[0]) == (T0 * 1000 + 7000, 1, (-70000) & 0xFFFFFFFFFFFFFFFF)
    assert (ts[1], kind[1], bits[1]) == (T0 * 1000 + 3599999, 1, 1 << 63)
    for s in range(8, 15):                                                   # the unsorted cells' planted maximum
        assert (ts[s], kind[s], bits[s]) == ((T0 + 3400) * 1000, 1, (-12345) & 0xFFFFFFFFFFFFFFFF)
    assert (ts[15], kind[15], bits[15]) == ((T0 + 3000) * 1000, 2, struct.unpack(">Q", struct.pack(">d", -2.25))[0])
    assert (ts[16], kind[16], bits[16]) == ((T0 + 3000) * 1000, 1, 99999)
    # the second hour of the last series is flagged only because of the first hour's datapoint at 3700 s
    _, flags, _, _, facts = IX.index_ref(b)
    assert not facts[-1].unsorted and flags[-1] & IX.ROW_UNSORTED and (flags[-1] >> IX.ROW_VL_SHIFT) & 0xF == 4
    sel = [n - 1]
    want = check_last(eng, b, sel, T0 + H + 10, None, 0, "flagged across rows", routes=(0, 0, 1, 0))
    assert (int(want[0][0]), int(want[2][0])) == ((T0 + H + 900) * 1000, 2)
    check_last(eng, b, sel, T0 + H + 10, None, 1, "flagged across rows, back scan", routes=(0, 0, 1, 0))
    check_last(eng, b, sel, T0 + 10, None, 0, "its first hour", routes=(1, 0, 0, 0))


@gpu
def test_walker_shaped_rows(eng):
    """3600-point float32 rows (tests/test_gpu_trim.py class_store("walker")): direct as routed,
    57 steps of the walk kernel under LAST_WALK=1."""
    from tests.test_gpu_trim import class_store
    pts, _, end = class_store("walker")
    b = load(eng, synth.from_series([p.rows() for p in pts], [0] * len(pts)))
    check_last(eng, b, None, end - 1, None, 0, "walker", routes=(len(pts), 0, 0, 0))
    check_last(eng, b, None, end + H, None, 2, "walker, an hour later", routes=(len(pts), 0, 0, 0))


# ---- the row lookup -------------------------------------------------------------------------------
@gpu
def test_row_lookup(eng):
    b = load(eng, lookup_store())
    last = T0 + 24 * 3 * H
    for anchor in (T0, T0 + 1, T0 + H - 1, T0 + 1800, T0 + H, T0 - 1, 0, T0 + 2 * H + 59, T0 + 23 * H, T0 + 24 * H, T0 + 25 * H,
                   T0 + 72 * H - 1, last, last + 5 * H, last + 1000 * H + 17, (1 << 32) + 5, (1 << 40)):
        for bs in (0, 1, 2, 3, 22, 23, 24, 1000, INT32_MAX):
            check_last(eng, b, None, anchor, None, bs, f"anchor {anchor - T0} back_scan {bs}")
    # exactly the distance, and one less
    sel = [10, 11]                                                          # 25 rows, consecutive / every third hour
    for s, gap in zip(sel, (1, 3)):
        top = T0 + 24 * gap * H
        for d in (1, 7, 1023):
            want = check_last(eng, b, [s], top + d * H + 3599, None, d, f"series {s} distance {d}", routes=(1, 0, 0, 0))
            assert int(want[0][0]) == (top + 7 * 24 % 3600) * 1000
            check_last(eng, b, [s], top + d * H, None, d - 1, f"series {s} distance {d} less one", routes=(0, 0, 0, 1))
    # a gap between rows: the anchor in the gap, the back scan reaching across it or not
    check_last(eng, b, [11], T0 + 5 * H + 100, None, 1, "in the gap, short", routes=(0, 0, 0, 1))
    check_last(eng, b, [11], T0 + 5 * H + 100, None, 2, "in the gap, reaching", routes=(1, 0, 0, 0))
    # per-series anchors
    rng = np.random.default_rng(8)
    each = (T0 + rng.integers(-2 * H, 80 * H, b.n_series)).tolist()
    for bs in (0, 2, 100):
        check_last(eng, b, None, 0, each, bs, f"anchors of their own, back_scan {bs}")
    each[3] = T0 + 3
    want = check_last(eng, b, None, T0 + 99 * H, each, 0, "anchor_s is not used beside anchor_each")
    assert int(want[2][2]) == (1 if T0 <= each[2] < T0 + H else 0)


# ---- the selection --------------------------------------------------------------------------------
@gpu
def test_selection(eng):
    b = load(eng, direct_store())
    n = b.n_series
    rng = np.random.default_rng(9)
    for n_sel in (0, 1, 64, 65, 257):
        sel = rng.integers(0, n, n_sel).tolist()                             # shuffled, with repeats
        check_last(eng, b, sel, T0, None, 0, f"n_sel {n_sel}", routes=(n_sel, 0, 0, 0))
    check_last(eng, b, list(range(n - 1, -1, -1)), T0, None, 0, "reversed")
    check_last(eng, b, None, T0 + H, None, 0, "null selection, an hour late", routes=(0, 0, 0, n))
    for bad in ([n], [-1], [0, 1, n + 7]):
        with pytest.raises(E.EngineError) as x:
            eng.last(bad, T0)
        assert x.value.code == abi.TSDB_E_ILLEGAL_ARGUMENT
    for kw in (dict(back_scan=-1), dict(anchor_s=-1), dict(anchor_each=[T0, -5], series_index=[0, 1])):
        with pytest.raises(E.EngineError) as x:
            eng.last(**{"series_index": [0], "anchor_s": T0, **kw})
        assert x.value.code == abi.TSDB_E_ILLEGAL_ARGUMENT
    import ctypes as C
    ts = np.zeros(n, np.int64)
    L = E.lib()
    IA = abi.TSDB_E_ILLEGAL_ARGUMENT
    assert L.tsdbhip_last(eng.ctx, None, n - 1, T0, None, 0, ts.ctypes.data, ts.ctypes.data, ts.ctypes.data, None) == IA
    assert L.tsdbhip_last(eng.ctx, None, n, T0, None, 0, ts.ctypes.data, None, ts.ctypes.data, None) == IA
    # the outputs of a call hold every selected slot and nothing beyond them
    guard = np.full(n + 8, -7, np.int64)
    bits, kind = np.full(n + 8, 7, np.uint64), np.full(n + 8, 9, np.uint8)
    sel = np.arange(n, dtype=np.int64)
    assert L.tsdbhip_last(eng.ctx, sel.ctypes.data, n, T0, None, 0, guard.ctypes.data, bits.ctypes.data, kind.ctypes.data, None) == 0
    assert (guard[n:] == -7).all() and (bits[n:] == 7).all() and (kind[n:] == 9).all() and (kind[:n] != 9).all()
    check_last(eng, b, None, T0, None, 0, "after the refused calls", routes=(n, 0, 0, 0))


@gpu
def test_more_answers_than_the_walk_grid_has_waves(eng):
    waves = walk_grid_waves()
    n = waves + waves // 8 + 3
    rng = np.random.default_rng(10)
    offs, vals = rng.integers(0, 3600, n), rng.integers(-30000, 30000, n)
    b = load(eng, synth.from_series([[one_point(T0 + (i % 3) * H, int(o), int(x))] for i, (o, x) in enumerate(zip(offs, vals))], [0] * n))
    want = R.last_ref(b, None, T0 + 2 * H, None, 2)
    assert (want[2] == 1).all() and np.array_equal(want[1].astype(np.int64), vals)
    with E.options(LAST_WALK=1):
        ts, bits, kind, info = eng.last(None, T0 + 2 * H, None, 2)
    for g, w in zip((ts, bits, kind), want):
        np.testing.assert_array_equal(g, w)
    assert (info.walked, info.direct, info.copied, info.none) == (n, 0, 0, 0) and n > waves
    ts, bits, kind, info = eng.last(None, T0 + 2 * H, None, 2)
    for g, w in zip((ts, bits, kind), want):
        np.testing.assert_array_equal(g, w)
    assert (info.walked, info.direct, info.copied, info.none) == (0, n, 0, 0)


# ---- life cycle -----------------------------------------------------------------------------------
def cycle_points():
    """Ten series over four hours: float32, small integers (the copy), wide integers, millisecond
    qualifiers, varying types (walked); series 7 stops after two hours, series 8 starts in the third."""
    rng = np.random.default_rng(12)
    pts = []
    for s in range(10):
        lo, hi = (0, 4 * H) if s not in (7, 8) else (0, 2 * H) if s == 7 else (2 * H, 4 * H)
        ts = T0 + np.arange(lo, hi, 97 + 13 * s)
        if s % 5 == 0:
            pts.append(quarter_points(rng, ts))
        elif s % 5 == 1:
            pts.append(int_points(rng, ts, -300, 300))
        elif s % 5 == 2:
            pts.append(int_points(rng, ts, -(1 << 40), 1 << 40))
        elif s % 5 == 3:
            pts.append(int_points(rng, ts, -100, 100, ms=True))
        else:
            kind = rng.integers(0, 3, len(ts))
            pts.append(Points(ts * 1000, lvals=rng.integers(-70000, 70000, len(ts)), fvals=rng.integers(1, 999, len(ts)) * 0.5, kind=kind))
    return pts


GIDS = [0, 1, NONE, 0, 1, 2, EXCL, 2, 0, 1]          # a regroup's ids
LOAD_GIDS = [0, 1, NONE, 0, 1, 2, NONE, 2, 0, 1]     # a load's
QS = [dsq(T0, T0 + 4 * H, "sum", "sum", 600000), dsq(T0, T0 + 4 * H, "none", "max", 600000)]


def check_cycle(eng, batch, ctx):
    """The resident batch is `batch`: every series at several anchors, and the call reads only."""
    before = [eng.run(q) for q in QS]
    rng = np.random.default_rng(13)
    for anchor, bs in ((T0 + 4 * H - 1, 0), (T0 + 4 * H - 1, 3), (T0 + 2 * H + 5, 1), (T0 + 9 * H, INT32_MAX), (T0 + H, 0)):
        check_last(eng, batch, None, anchor, None, bs, f"{ctx} anchor {anchor - T0} back_scan {bs}")
    sel = rng.integers(0, batch.n_series, 23).tolist()
    check_last(eng, batch, sel, 0, (T0 + rng.integers(0, 5 * H, 23)).tolist(), 1, f"{ctx} subset")
    for i, (x, q) in enumerate(zip(before, QS)):
        identical(x, eng.run(q), f"{ctx} q{i} after tsdbhip_last")


@gpu
def test_after_regroup(eng):
    pts = cycle_points()
    a = load(eng, synth.from_series([p.rows() for p in pts], [0] * len(pts)))
    eng.regroup(GIDS)
    check_cycle(eng, a, "regroup")
    want = check_last(eng, a, [6], T0 + 4 * H - 1, None, 0, "the excluded series")   # exclusion is a query's state
    assert int(want[2][0]) != 0
    eng.regroup([EXCL] * len(pts))
    check_cycle(eng, a, "every series excluded")


@gpu
def test_after_append_replaced_the_live_hour(eng):
    pts = cycle_points()
    a, d, idx, new, full = split(pts, LOAD_GIDS, T0 + 3 * H + 1700, resident=[s != 8 for s in range(10)])
    load(eng, a)
    check_cycle(eng, a, "before the append")
    info = eng.append(d, idx, new)
    assert info.rows_replaced > 0 and info.series_added == 1
    m = merge_batches(a, d, idx, new)
    check_cycle(eng, m, "append")
    old_of_new = [i for i in range(10) if i != 8]                            # the live hour's answers moved on
    assert (R.last_ref(m, old_of_new, T0 + 4 * H - 1)[0] > R.last_ref(a, None, T0 + 4 * H - 1)[0]).sum() >= 8


@gpu
def test_after_upsert_into_a_closed_hour(eng):
    pts = cycle_points()
    a = load(eng, synth.from_series([p.rows() for p in pts], LOAD_GIDS))
    # late datapoints for hour 1 of series 1 (the copy), 2 and 4; a back-filled hour 1 for series 8
    rng = np.random.default_rng(14)
    late = {1: int_points(rng, T0 + H + np.arange(0, H, 41), -300, 300), 2: int_points(rng, T0 + H + np.arange(5, H, 400), -9, 1 << 50),
            4: quarter_points(rng, T0 + H + np.arange(0, H, 1000)), 8: int_points(rng, T0 + H + np.arange(3, H, 500), 0, 9, ms=True)}
    d = synth.from_series([late[s].rows() for s in sorted(late)], [LOAD_GIDS[s] for s in sorted(late)])
    info = eng.upsert(d, sorted(late), [0] * len(late))
    assert info.rows_replaced == 3 and info.rows_added == 1
    m = merge_batches(a, d, sorted(late), [0] * len(late))
    check_cycle(eng, m, "upsert")
    want = check_last(eng, m, sorted(late), T0 + H + 10, None, 0, "the upserted hour")
    assert want[0].tolist() == [int(late[s].ts[-1]) for s in sorted(late)]


@gpu
@pytest.mark.parametrize("pack", [NO_PACK, 0], ids=["nopack", "pack"])
def test_after_trim(eng, pack):
    pts = cycle_points()
    a = load(eng, synth.from_series([p.rows() for p in pts], LOAD_GIDS))
    eng.trim(T0 + 2 * H, pack)
    t = trim_batch(a, T0 + 2 * H)
    check_cycle(eng, t, f"trim {pack}")
    check_last(eng, t, [7], T0 + 4 * H, None, INT32_MAX, "a series left without rows", routes=(0, 0, 0, 1))


@gpu
@pytest.mark.parametrize("drop", [False, True], ids=["keep", "drop"])
@pytest.mark.parametrize("pack", [NO_PACK, 0], ids=["nopack", "pack"])
def test_after_remove(eng, pack, drop):
    pts = cycle_points()
    a = load(eng, synth.from_series([p.rows() for p in pts], LOAD_GIDS))
    ranges = [(0, T0 + 3 * H, T0 + 4 * H), (1, T0 + H, T0 + 3 * H), (4, T0 + 3 * H, T0 + 3 * H + 1), (7, 0, 1 << 32), (8, T0 + 2 * H, T0 + 3 * H),
              (1, T0, T0 + 4 * H)]                                           # series 1 and 7 are left without rows
    info, new_index = eng.remove(ranges, drop, pack)
    t, want_index = remove_batch(a, ranges, drop)
    np.testing.assert_array_equal(new_index, want_index)
    assert t.n_series == (8 if drop else 10)
    check_cycle(eng, t, f"remove {pack} {drop}")
    kept = [i for i in range(10) if new_index[i] >= 0]
    got = check_last(eng, t, [int(new_index[i]) for i in kept], T0 + 4 * H - 1, None, 3, "by the new indices")
    was = R.last_ref(remove_batch(a, ranges, False)[0], kept, T0 + 4 * H - 1, None, 3)
    for g, w in zip(got, was):
        np.testing.assert_array_equal(g, w)                                  # renumbering moves no answer


@gpu
def test_rollup_and_preagg_cells_stay(eng):
    pts = cycle_points()
    a = load(eng, synth.from_series([p.rows() for p in pts], LOAD_GIDS))
    iv = E.rollup_interval("10m", "1d")
    cells = eng.rollup(iv, T0, T0 + 4 * H, [("sum", 0)])
    n_cells, value_bytes = eng.rollup_run(iv, T0, T0 + 4 * H, [("sum", 0)])
    check_last(eng, a, None, T0 + 4 * H - 1, None, 2, "between rollup_run and its download")
    again = eng.rollup_download(n_cells, value_bytes)
    assert len(again) == len(cells) > 0
    for i in (0, len(cells) // 2, len(cells) - 1):
        assert again.cell(i) == cells.cell(i)


# ---- errors ---------------------------------------------------------------------------------------
@gpu
def test_malformed_answer_row(eng):
    good = one_point(T0, 5, 1)
    bad = (T0 + H, q2(0, 0) + q2(10, 2) + q2(20, 1), b"\x01\x00\x01\x02\x00\x03\x00")   # a 3-byte integer among others
    b = load(eng, synth.from_series([[good, bad, one_point(T0 + 2 * H, 9, 3)], [one_point(T0 + H, 1, 2)]], [0, 0]))
    assert predict(b, None, T0 + H + 5, None, 0) is None
    for walk in (None, 1):
        with E.options(LAST_WALK=walk):
            for sel, anchor, bs in ((None, T0 + H + 5, 0), ([1, 0], T0 + H, 3), ([0], T0 + H + 3599, INT32_MAX)):
                with pytest.raises(E.EngineError) as x:
                    eng.last(sel, anchor, None, bs)
                assert x.value.code == abi.TSDB_E_ILLEGAL_DATA and x.value.java == "IllegalDataException"
    # the same store with that row outside the window: newer than the anchor hour, older than the answer row, not selected
    check_last(eng, b, None, T0 + 100, None, 0, "before the malformed row", routes=(2 - 1, 0, 0, 1))
    check_last(eng, b, None, T0 + 2 * H, None, 5, "after it", routes=(2, 0, 0, 0))
    check_last(eng, b, [1, 1], T0 + H, None, 0, "beside it", routes=(2, 0, 0, 0))


@gpu
def test_not_implemented_contexts(eng):
    from opentsdb_amd.rollup_read import make_rollup_batch
    NI = abi.TSDB_E_NOT_IMPLEMENTED
    b = lookup_store()

    def code(e, sel=(0,)):
        try:
            e.last(list(sel), T0)
        except E.EngineError as x:
            return x.code, str(x)
        return 0, ""

    fresh = E.Engine(0)
    try:
        assert code(fresh)[0] == NI and "tsdbhip_load" in code(fresh)[1]
    finally:
        fresh.close()
    iv = E.rollup_interval("10m", "1d")
    rcell = (struct.pack(">H", (0 << 4) | 0x7), struct.pack(">q", 5))
    eng.load_rollup(make_rollup_batch([(None, [(T0, [rcell], [])])], [0], iv, False))
    assert code(eng)[0] == NI and "rollup batch" in code(eng)[1]
    eng.load_shard(b, E.SHARD_SPANS, 0, b.n_series)
    assert code(eng)[0] == NI
    md = E.Engine(devices=[0, 0])
    try:
        md.load(b)
        assert code(md)[0] == NI and "multi-device" in code(md)[1]
    finally:
        md.close()
    load(eng, b)
    check_last(eng, b, None, T0 + 3 * H, None, 1, "after the refusals")


# ---- ResidentSpans.last on the engine -------------------------------------------------------------
@gpu
def test_resident_spans_last(eng):
    from opentsdb_amd.query import ResidentSpans
    from tests.test_regroup_cpu import END, METRIC, START, TAGS, make_store
    from tests.test_last_cpu import expected, tsuid
    st = make_store()
    rs = ResidentSpans(st, METRIC, START, END, engine=eng)
    subs = [{"tsuids": [tsuid(st, TAGS[3]), tsuid(st, TAGS[4])]}, {"metric": METRIC, "tags": TAGS[5]}, {"metric": METRIC, "tags": {"host": "nobody"}}]
    out = rs.last(subs, back_scan=0, now_s=END - 1)
    assert [(p.tsuid, p.timestamp, p.value) for p in out] == [(tsuid(st, t), *expected(st, t, END - 1, 0)) for t in (TAGS[3], TAGS[5])]
    out = rs.last(subs, back_scan=3, now_s=END - 1)
    assert [(p.tsuid, p.timestamp, p.value) for p in out] == [(tsuid(st, t), *expected(st, t, END - 1, 3)) for t in (TAGS[3], TAGS[4], TAGS[5])]
