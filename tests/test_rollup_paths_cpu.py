"""The rollup route stores are what they claim to be, before any GPU sees them (no device
needed): their row classes, the bucket runs per chunk and per lane each case is named for, the
side of the streaming pass's LDS limit each window lies on, and a few cells computed by hand
that pin oracle/rollup.generate on the new geometry (1 s cells, a window end inside a bucket,
points one millisecond either side of a bucket boundary)."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import rollup as R
from tests import index_ref as IR
from tests import rollup_paths as P


def facts_by_series(batch):
    ndp, flags, lsb, absmax, facts = IR.index_ref(batch)
    srp = np.asarray(batch.series_row_ptr).astype(int)
    return [[(facts[r], int(flags[r])) for r in range(srp[s], srp[s + 1])] for s in range(len(srp) - 1)]


def is_class(f, fl, qw, vl):
    """The row is of the streaming class (qw, vl) (kcommon.h fast_row_ok, min / max form)."""
    if f.err or fl & IR.ROW_UNSORTED or f.qw != qw:
        return False
    if vl == 0:
        return f.alli and f.vle2
    return f.vl == vl and f.allf and not f.nan and not f.negz


# ---- row classes ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.CERTIFIED + P.UNCERTIFIED)
def test_uniform_store_is_one_class(name):
    b = P.uniform(name)
    assert P.n_points(b) <= 45000
    qw, vl = P.CLASS_OF[name]
    for rows in facts_by_series(b):
        assert len(rows) == 3
        for f, fl in rows:
            assert is_class(f, fl, qw, vl), (name, f)
            assert bool(fl & IR.ROW_NOCERT) == (name in P.UNCERTIFIED)
        # a 5-second first row, a full row, a partial last row
        period = P.SPAN_S * 1000 // sum(f.ndp for f, _ in rows)
        assert rows[0][0].ndp == -(-5000 // period) and rows[2][0].ndp < rows[1][0].ndp
    mid = facts_by_series(b)[0][1][0].ndp
    if name == "vle8s":
        assert mid == 450 and mid <= P.CH
    if name == "vle7s":
        assert mid in (514, 515) and mid > P.CH          # k_rollup_fast<2, 0> hands the row back
    if name in ("q2f32", "q2f64", "fm1s"):
        assert mid == 3600 == 7 * P.CH + 16              # 7 full chunks and a partial one


def test_chain_store_classes():
    b = P.chain()
    assert P.n_points(b) <= 45000
    rows = dict(zip((n for n, _ in P.CHAIN_SERIES), facts_by_series(b)))
    gid = dict(P.CHAIN_SERIES)
    dp = {"A": 0, "B": 0, "q4f64": 0, "q2f64": 0}
    for name, rr in rows.items():
        assert len(rr) == 3
        if gid[name] < 0:
            continue
        for f, fl in rr:
            dp["A"] += f.ndp * is_class(f, fl, 2, 4)
            dp["B"] += f.ndp * (is_class(f, fl, 2, 0) and f.ndp <= P.CH)
            dp["q4f64"] += f.ndp * is_class(f, fl, 4, 8)
            dp["q2f64"] += f.ndp * is_class(f, fl, 2, 8)
    # the engine ranks the classes by datapoints: float32 first, vle second, the others left over
    assert dp["A"] > dp["B"] > max(dp["q4f64"], dp["q2f64"]) > 0, dp
    for name in ("f32_a", "f32_b", "f32_c", "f32_d", "nogroup"):
        assert all(is_class(f, fl, 2, 4) and not fl & IR.ROW_NOCERT for f, fl in rows[name])
    for name in ("vle_a", "vle_b", "vle_c"):
        assert all(is_class(f, fl, 2, 0) and f.ndp <= P.CH for f, fl in rows[name])
    for name in ("q4f64_a", "q4f64_b"):
        assert all(is_class(f, fl, 4, 8) and not fl & IR.ROW_NOCERT for f, fl in rows[name])
    assert all(is_class(f, fl, 2, 8) and fl & IR.ROW_NOCERT for f, fl in rows["fm"])
    # the late breakers: class A in rows 0 and 1, not in row 2
    for name in P.CHAIN_LATE:
        assert all(is_class(f, fl, 2, 4) for f, fl in rows[name][:2]), name
        assert not is_class(*rows[name][2], 2, 4), name
    f, fl = rows["late_nan"][2]
    assert f.nan and fl & IR.ROW_NAN and f.qw == 2 and f.vl == 4
    f, fl = rows["late_int4"][2]
    assert f.qw == 2 and f.vl == 4 and not f.allf and not f.alli
    f, fl = rows["late_ms"][2]
    assert f.qw == 0 and f.allf
    # batch order is not group order, and the series without a group sits in the middle
    g = [x for _, x in P.CHAIN_SERIES]
    assert g != sorted(g) and 0 < g.index(-1) < len(g) - 1


def test_nan_store_rows():
    b = P.nans()
    rows = facts_by_series(b)
    assert all(is_class(f, fl, 2, 4) for s in (0, 1) for f, fl in rows[s])
    for s in range(2, 8):
        assert all(f.nan and fl & IR.ROW_NAN and f.qw == 2 and f.vl == 4 for f, fl in rows[s][1:])
    # series 2: no value at all in its second row (absmax stays 0, no lsb)
    f, _ = rows[2][1]
    assert f.ndp == 1200 and f.absmax == 0.0 and f.lsb == IR.INT32_MAX


@pytest.mark.parametrize("name,ms", [("swap_dup", False), ("ms", True)])
def test_stored_order_stores_are_unsorted(name, ms):
    b = P.stored_order(name)
    rows = [x for rr in facts_by_series(b) for x in rr]
    n_uns = sum(1 for f, fl in rows if fl & IR.ROW_UNSORTED)
    assert n_uns >= 10 and n_uns < len(rows)
    assert any(f.qw != 2 for f, _ in rows) == ms


def test_boundary_store_rows():
    b = P.boundary()
    for rows in facts_by_series(b):
        assert len(rows) == 2 and all(is_class(f, fl, 4, 4) for f, fl in rows)
    for i, I in enumerate(P.BOUNDARY_I):
        ts = np.concatenate([t for _, t in P.series_points(b, 3 * i)])
        r = ts % (I * 1000)
        assert set(r.tolist()) == {0, 1, I * 1000 - 1}
        k = np.arange(P.H1 * 1000 // (I * 1000) + 1, (P.H1 + 7200) * 1000 // (I * 1000))
        for d in (-1, 0, 1):
            assert np.isin(k * I * 1000 + d, ts).all()


# ---- K per window: which side of the streaming pass's LDS limit ---------------------------------
def test_lds_limit_is_k_1170():
    assert P.rollup_fast_lds(P.K_FAST_MAX) <= 32 * 1024 < P.rollup_fast_lds(P.K_FAST_MAX + 1)


@pytest.mark.parametrize("interval,span", P.A_INTERVALS)
def test_case_a_window_side(interval, span):
    """K covers the scan's whole hour rows: 1s, 2s, 3s (3600, 1800, 1200 slots in the one row the
    window touches) and 5s (2 x 720: the window reaches the third row) are beyond the streaming
    pass; from 7s on the pass runs."""
    I = P.interval_seconds(interval)
    s, e = P.a_window(interval)
    K = P.window_k(I, s, e)
    assert K == {"1s": 3600, "2s": 1800, "3s": 1200, "5s": 1440, "7s": 1029, "13s": 831, "45s": 160, "90s": 80,
                 "1m": 120, "5m": 24, "1h": 2}[interval]
    assert P.streams(I, s, e) == (interval not in ("1s", "2s", "3s", "5s"))


@pytest.mark.parametrize("interval,span,win", P.A_SHORT)
def test_short_window_streams(interval, span, win):
    I = P.interval_seconds(interval)
    K = P.window_k(I, *win)
    assert K <= P.K_FAST_MAX and (K == 3600 // I or interval == "13s")
    assert R.generate(P.uniform("q2f32"), R.Interval(interval, span), *win, (("count", 1),))   # (not refused)


@pytest.mark.parametrize("interval,span", P.C_INTERVALS)
def test_case_c_window_sides(interval, span):
    """Small K: the window inside the second row; large K: 1s anywhere, and 7s, 8s and 9s
    over all three rows (1543, 1350 and 1200 slots)."""
    I = P.interval_seconds(interval)
    small, large = (P.streams(I, *w) for w in P.C_WINDOWS)
    assert small == (interval != "1s")
    assert large == (interval not in ("1s", "7s", "8s", "9s"))


def test_other_windows_sides():
    assert not P.streams(1, P.START, P.END) and P.window_k(1, P.START, P.END) == 3 * 3600   # case b
    assert P.window_k(7, P.WIN0, P.END) == 1029 and P.window_k(60, P.START, P.END) == 180      # case d
    assert P.window_k(7, *P.BOUNDARY_WINDOW) == 1029 and P.window_k(45, *P.BOUNDARY_WINDOW) == 160   # case h
    assert P.window_k(3, P.START, P.END) == 3600 and P.window_k(60, P.START, P.END) <= P.K_FAST_MAX   # case f


# ---- runs per chunk and per lane ---------------------------------------------------------------
def all_runs(batch, s, interval, win):
    return P.runs(batch, s, P.interval_seconds(interval), *win)


@pytest.mark.parametrize("interval", ["1s", "2s", "3s"])
def test_three_or_more_runs_in_every_lane(interval):
    """rfast_chunk emits the runs wholly inside a lane itself (1 s data, general kernel)."""
    rr = all_runs(P.uniform("q2f32"), 0, interval, P.a_window(interval))
    full = [lanes for _, lanes in rr if len(lanes) == 64]
    assert full and all(min(lanes) >= 3 for lanes in full[1:])


def test_split_vote_lanes_disagree():
    """5s on 1 s data: lanes with <= 2 and lanes with > 2 runs in one chunk, inside the streaming
    pass.  4s and 6s: two runs in every lane, the two-run fold with its threshold in every lane."""
    rr = all_runs(P.uniform("q2f32"), 0, "5s", P.SHORT_WINDOW)
    mixed = [lanes for _, lanes in rr if len(lanes) == 64 and min(lanes) <= 2 and max(lanes) >= 3]
    assert len(mixed) >= 6
    for iv in ("4s", "6s"):
        full = [lanes for _, lanes in all_runs(P.uniform("q2f32"), 0, iv, P.SHORT_WINDOW) if len(lanes) == 64]
        assert len(full) >= 7 and all(set(lanes) == {2} for lanes in full[1:])


@pytest.mark.parametrize("name,interval", [("vle8s", "7s"), ("vle8s", "13s"), ("vle8s", "45s"), ("q4f32", "1s")])
def test_streaming_per_datapoint_fold(name, interval):
    """More than two buckets in one lane's 8 datapoints (rf_chunk's per-datapoint fold)."""
    win = P.a_window(interval) if name == "vle8s" else P.SHORT_WINDOW
    rr = all_runs(P.uniform(name), 0, interval, win)
    assert any(max(lanes) >= 3 for _, lanes in rr)
    if name == "vle8s":
        assert P.streams(P.interval_seconds(interval), *win)


def test_runs_per_chunk_of_the_sequential_loop():
    """rslow_chunk: 512 runs (1s), 74 runs: a second, partial round (7s), exactly 64 runs in the
    aligned chunks (8s on 1 s data), 57 (9s)."""
    b = P.uniform("fm1s")
    win = (P.START, P.END)
    full = lambda iv: [n for n, lanes in all_runs(b, 0, iv, win) if len(lanes) == 64 and min(lanes) > 0]   # noqa: E731
    assert set(full("1s")) == {512}
    assert set(full("7s")) <= {74, 75} and 74 in full("7s")
    assert full("8s").count(64) >= 7 and set(full("8s")) == {64}
    assert set(full("9s")) <= {57, 58}
    b5 = P.uniform("fm500")
    n5 = [n for n, lanes in all_runs(b5, 0, "1s", win) if len(lanes) == 64]
    assert set(n5) == {256}                     # 500 ms data: four full rounds
    n5 = [n for n, lanes in all_runs(b5, 0, "8s", win) if len(lanes) == 64]
    assert set(n5) == {32}


def test_long_buckets_carry_across_chunks_and_rows():
    b = P.uniform("q2f32")
    one = [n for n, _ in all_runs(b, 0, "1h", (P.START, P.END))]
    assert len(one) == 1 + 8 + 2 and set(one) == {1}
    day = [n for n, _ in all_runs(b, 0, "1d", (P.START, P.END))]
    assert set(day) <= {0, 1}


# ---- hand-computed cells ------------------------------------------------------------------------
def points_of(batch, s):
    """(ts ms, float values) of a float32 series."""
    ts = np.concatenate([t for _, t in P.series_points(batch, s)])
    vals = []
    for r in range(int(batch.series_row_ptr[s]), int(batch.series_row_ptr[s + 1])):
        v = bytes(batch.val[int(batch.row_val_off[r]):int(batch.row_val_off[r + 1])])
        n = len(P.series_points(batch, s)[r - int(batch.series_row_ptr[s])][1])
        vals.append(np.frombuffer(v[:4 * n], ">f4").astype(np.float64))
    return ts, np.concatenate(vals)


def cell(iv, s, ts_s, fn_id, v, as_long):
    flags, vb = R.encode_value(float(v), as_long)
    base = R.basetime(ts_s, iv)
    return (s, base, R.qualifier(ts_s, base, flags, fn_id, iv), vb)


def test_cells_by_hand_1s():
    """Under 1 s cells each cell is its datapoint."""
    b = P.uniform("q2f32")
    iv = R.Interval("1s", "1h")
    s0, e0 = P.WIN0, P.WIN0 + 40
    got = R.generate(b, iv, s0, e0, (("sum", 0), ("count", 1)))
    want = []
    for fn, fid in (("sum", 0), ("count", 1)):
        for s in range(6):
            ts, v = points_of(b, s)
            for t, x in zip(ts, v):
                if s0 * 1000 <= t < e0 * 1000:
                    want.append(cell(iv, s, int(t) // 1000, fid, x if fn == "sum" else 1, fn == "count"))
    assert got == want and len(got) == 2 * 6 * 40


def test_cells_by_hand_unaligned_window_end():
    """A window that ends 30 s into a minute: the last bucket starts before the end and holds
    the whole minute's 60 points, those after the end as well."""
    b = P.uniform("q2f32")
    iv = R.Interval("1m", "1h")
    end = P.H1 + 600 + 30
    got = R.generate(b, iv, P.H1 + 540, end, (("sum", 0), ("count", 1), ("max", 2), ("min", 3)))
    ts, v = points_of(b, 0)
    want = []
    for fid, f in ((0, np.sum), (1, len), (2, np.max), (3, np.min)):
        for s in range(6):
            ts, v = points_of(b, s)
            for b0 in (P.H1 + 540, P.H1 + 600):
                x = v[(ts >= b0 * 1000) & (ts < (b0 + 60) * 1000)]
                assert len(x) == 60
                acc = 0.0
                for y in x:          # Java's left-to-right sum
                    acc += y
                want.append(cell(iv, s, b0, fid, acc if fid == 0 else f(x), fid == 1))
    assert got == want


@pytest.mark.parametrize("i,I,span", [(0, 7, "2h"), (1, 45, "1h")])
def test_cells_by_hand_boundary(i, I, span):
    """The first three buckets of a boundary series: the points k*I and k*I + 1 ms open bucket k,
    (k + 1)*I - 1 ms closes it."""
    b = P.boundary()
    iv = R.Interval(f"{I}s", span)
    s = 3 * i
    ts, v = points_of(b, s)
    k0 = -(-P.H1 // I)
    got = [c for c in R.generate(b, iv, P.H1, P.H1 + 7200, (("sum", 0), ("count", 1))) if c[0] == s]
    at = dict(zip(ts.tolist(), v.tolist()))
    for j in range(3):
        t = (k0 + j) * I
        vals = [at[t * 1000], at[t * 1000 + 1], at[(t + I) * 1000 - 1]]
        assert cell(iv, s, t, 0, (vals[0] + vals[1]) + vals[2], False) in got[:3]
        assert cell(iv, s, t, 1, 3, True) in got
    assert got[0] == cell(iv, s, k0 * I, 0, (at[k0 * I * 1000] + at[k0 * I * 1000 + 1]) + at[(k0 + 1) * I * 1000 - 1], False)
