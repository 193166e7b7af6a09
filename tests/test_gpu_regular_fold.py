"""The closed-form chunk fold of regular rows (`fast_chunk_reg`, DESIGN §5.1 "Regular rows").

For a regular row the datapoints of a chunk lie at n = nA + i * su (su = step * uq n-units), so the
REG kernels decide per chunk, on scalars, whether the chunk lies inside the slot range and whether
a lane's 8 points can span more than two buckets (7 * su <= In), and per lane take one division by
the interval, the distance to the next bucket boundary and the first run's length by arithmetic.
The cases below sit where that arithmetic can go wrong.  Every case is held two ways: REG against
option REGULAR = 0 bit for bit (`both`, which also asserts that REG tiles were launched), and
against the oracle.
(1 s buckets alone are held without the REG assertion: the engine sends them to k_grid.)
"""
from __future__ import annotations

import numpy as np
import pytest

from opentsdb_amd import abi, synth
from opentsdb_amd import engine as E
from oracle import oracle as O
from tests.test_gpu_parity import assert_groups_match, T0
from tests.test_gpu_regroup import agg_name, dsq
from tests.test_gpu_regular import FAST_FNS, ap, both, fcell, quarters, regular_store

pytestmark = pytest.mark.gpu

H = 3600
END = T0 + 2 * H
NPTS = [1, 2, 8, 9, 511, 512, 513, 1024, 1025]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


_stores = {}


def cached(key, make):
    if key not in _stores:
        _stores[key] = make()
    return _stores[key]


def step_store(step, vl=4, step2=None):
    return cached(("step", step, vl, step2), lambda: regular_store(70, 3, vl, seed=300 + step + vl, step=step, step2=step2))


def lens_store():
    """81 series of a long row (hour 0, 600 points at step 3) and a row of every length in NPTS
    (hour 1) at steps 1, 2 and 3 whose first offset is 0, 1 or the one that puts the last point at
    3599: partial last lanes, partial last chunks, exact chunk multiples."""
    def make():
        rng = np.random.default_rng(77)
        series = []
        for n in NPTS:
            for st in (1, 2, 3):
                for first in (0, 1, 3599 - (n - 1) * st):
                    rows = []
                    for h, offs in ((0, ap(len(series) % 5, 3, 600)), (1, ap(first, st, n))):
                        q, v = fcell(offs, quarters(rng, len(offs)))
                        rows.append((T0 + h * H, q, v))
                    series.append(rows)
        return synth.from_series(series, [s % 4 for s in range(len(series))])
    return cached("lens", make)


def check(eng, store, q, ctx, tol=None, streamed=True):
    """streamed: the streaming kernels took the query (`both` reads the REG tiles of the last
    streaming launch; a query the engine keeps off that path hands every tile to k_grid)."""
    got = both(eng, lambda: eng.run(q), ctx, expect_reg=streamed)
    t = eng.timing()
    assert (t.redo_tiles < t.tiles) == streamed, f"{ctx}: {t.redo_tiles} of {t.tiles} tiles through k_grid"
    assert_groups_match(got, O.run_query(store, q), agg_name(q), tol=tol, ctx=f"{ctx} vs oracle")


def msq(start_ms, end_ms, agg, fn, interval_ms, **kw):
    return abi.new_query(start_ms, end_ms, agg, ds_function=abi.AGG[fn], ds_interval_ms=interval_ms, **kw)


# ---- 1. a lane's span against the bucket width ---------------------------------------------------
@pytest.mark.parametrize("step,secs", [(1, (6, 7, 8)), (10, (60, 70, 80))], ids=["step1", "step10"])
def test_lane_span(eng, step, secs):
    """7 * step one above, equal to and one below the interval: the scalar "at most two buckets a
    lane" test flips between the per-datapoint loop and the closed form."""
    # (a row of step 10 has 360 points: it rides in the walker's tile as the second row beside a long one)
    b, at = (step_store(1), T0 + 100) if step == 1 else (step_store(3, step2=step), T0 + H)
    eng.load(b)
    for s in secs:
        for fn in ("sum", "avg", "min"):
            # K <= 64 (register partials) inside one row, and the whole range (LDS partials)
            check(eng, b, dsq(at, at + 45 * s, "sum", fn, 1000 * s), f"step {step} {s}s-{fn} window")
        check(eng, b, dsq(T0, END, "sum", "avg", 1000 * s), f"step {step} {s}s-avg whole range")


def test_lane_over_two_buckets(eng):
    """Step 61 under 1m buckets: a lane's 8 points span 427 s."""
    b = step_store(3, step2=61)
    eng.load(b)
    for fn in ("sum", "count", "max"):
        check(eng, b, dsq(T0, END, "sum", fn, 60000), f"step 61 1m-{fn}")
        check(eng, b, dsq(T0 + H + 100, T0 + H + 3500, "sum", fn, 60000), f"step 61 1m-{fn} second row")


# ---- 2. both units --------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 3])
def test_millisecond_units(eng, step):
    """Intervals that are no whole seconds, and a start that is none: n-units are milliseconds
    (uq = 1000).  1500 / 2500 ms buckets are narrower than a lane (per datapoint); 7000 * step and
    above take the closed form with su = 1000 * step."""
    b = step_store(step)
    eng.load(b)
    t0 = (T0 + 700) * 1000
    for iv in (1500, 2500):
        check(eng, b, msq(t0 + 250, t0 + 60 * iv + 750, "sum", "sum", iv), f"step {step} {iv}ms K<=64")
        check(eng, b, msq(t0 + 250, t0 + 100 * iv + 750, "sum", "avg", iv), f"step {step} {iv}ms K>64")
    for iv in (7000 * step - 500, 7000 * step + 500, 10500 * step, 60000):
        for fn in ("sum", "avg", "count"):
            check(eng, b, msq(t0 + 250, t0 + 50 * iv + 750, "sum", fn, iv), f"step {step} {iv}ms-{fn} ms start")
    # second-aligned buckets from a start that is not a whole second, over both rows
    check(eng, b, msq(T0 * 1000 + 1, END * 1000 - 2, "sum", "avg", 60000), f"step {step} 1m ms start whole range")
    check(eng, b, msq((T0 + 1234) * 1000 + 999, (T0 + H + 2345) * 1000 + 1, "sum", "sum", 90000), f"step {step} 90s ms edges")


# ---- 3. the division, row lengths and first offsets -----------------------------------------------
def test_division_and_row_lengths(eng):
    b = lens_store()
    eng.load(b)
    assert 70 <= b.n_series <= 131
    for s in (59, 60, 61, 3599, 3600, 7200):
        for fn in ("sum", "avg"):
            check(eng, b, dsq(T0, END, "sum", fn, 1000 * s), f"lengths {s}s-{fn}")
    # narrow buckets over windows of the second hour, where the rows of every length lie:
    # its start (first 0 / 1), the chunk edges at 512 and 1024 points, and the hour's end
    for s, span in ((2, 128), (3, 190), (7, 440)):
        for at in (0, 480, 1000, H - span):
            q = dsq(T0 + H + at, T0 + H + at + span, "sum", "sum", 1000 * s)
            check(eng, b, q, f"lengths {s}s at {at}")
    check(eng, b, dsq(T0 + H, T0 + H + 128, "sum", "count", 2000), "lengths 2s-count K 64")
    # 1 s buckets: the engine keeps them off the streaming kernels (every tile goes to k_grid, with
    # or without REGULAR), so no REG tile can be asked for; the results are held all the same
    for at in (0, 480, H - 64):
        check(eng, b, dsq(T0 + H + at, T0 + H + at + 64, "sum", "sum", 1000), f"lengths 1s at {at}", streamed=False)
    check(eng, b, dsq(T0, END, "sum", "count", 60000), "lengths 1m-count K 120")
    check(eng, b, dsq(T0, END, "max", "max", 120000), "lengths 2m-max")


# ---- 4. the edges of the slot range ---------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 7])
def test_range_edges(eng, step):
    """Start inside the first row (n0 < 0 for the leading lanes of a chunk) and end inside the last
    (slots >= K for the trailing ones): those chunks take the per-datapoint loop, their
    neighbours the closed form."""
    b = step_store(step)
    eng.load(b)
    for fn in FAST_FNS:
        check(eng, b, dsq(T0 + 1234 * step % 3000, T0 + H + 345 * step, "sum", fn, 60000), f"step {step} 1m-{fn} inside the rows")
    check(eng, b, dsq(T0 + 3, T0 + H + 500, "sum", "avg", 120000), f"step {step} 2m start in the first lane")
    check(eng, b, dsq(T0 + 517 * step, T0 + 517 * step + 120, "sum", "sum", 2000), f"step {step} 2s around a chunk edge")


# ---- 5. every function and form -------------------------------------------------------------------
@pytest.mark.parametrize("step,vl", [(1, 4), (1, 8), (7, 4), (7, 8)], ids=lambda v: str(v))
def test_every_form(eng, step, vl):
    b = step_store(step, vl)
    eng.load(b)
    for fn in FAST_FNS:                                   # KR 1: the plain group-by, K = 60
        check(eng, b, dsq(T0, END, "sum", fn, 120000), f"step {step} vl {vl} sum:2m-{fn}")
    qs = [dsq(T0, END, a, "avg", 120000) for a in ("avg", "min", "max", "count", "dev")]   # KR 2
    multi = both(eng, lambda: eng.run_multi(qs), f"step {step} vl {vl} run_multi")
    for q, g in zip(qs, multi):
        assert_groups_match(g, O.run_query(b, q), agg_name(q), ctx=f"step {step} vl {vl} run_multi {agg_name(q)} vs oracle")
    check(eng, b, dsq(T0, END, "p99", "avg", 120000), f"step {step} vl {vl} p99:2m-avg", tol=0.0)   # KR 3
    check(eng, b, dsq(T0, END, "sum", "sum", 120000, flags=abi.QF_ORDERED), f"step {step} vl {vl} ordered sum:2m-sum")
    check(eng, b, dsq(T0, END, "sum", "avg", 120000, rate=True), f"step {step} vl {vl} rate sum:2m-avg")   # KR 0
    for fn in FAST_FNS:
        check(eng, b, dsq(T0, END, "sum", fn, 60000), f"step {step} vl {vl} sum:1m-{fn} K 120")


# ---- 6. counts ------------------------------------------------------------------------------------
def test_counts(eng):
    """Step 7 under 1m buckets: 8 and 9 points a bucket."""
    assert set(np.bincount(ap(0, 7, 515) // 60).tolist()) == {8, 9}   # (a row of regular_store at step 7)
    b = step_store(7)
    eng.load(b)
    for agg in ("sum", "max"):
        for fn in ("count", "avg"):
            check(eng, b, dsq(T0, END, agg, fn, 60000), f"step 7 {agg}:1m-{fn}")
            check(eng, b, dsq(T0 + 60, T0 + 3660, agg, fn, 60000), f"step 7 {agg}:1m-{fn} K 60")


# ---- 7. hand-back ---------------------------------------------------------------------------------
def test_certificate_hand_back_fold(eng):
    """A series whose bucket sums cannot be certified goes from the closed-form fold to k_grid."""
    b = cached("big", lambda: regular_store(70, 3, 4, seed=9, step=1, big=(11, 40)))
    eng.load(b)
    for q in (dsq(T0, END, "sum", "sum", 60000), dsq(T0, END, "sum", "avg", 120000)):
        got = both(eng, lambda: eng.run(q), "certificate")
        assert eng.timing().redo_tiles >= 2, "the uncertified series were not handed back"
        assert_groups_match(got, O.run_query(b, q), "sum", ctx="certificate vs oracle")
