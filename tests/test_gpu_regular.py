"""Regular rows: the per-row {first, step} side array of the index, the regular tile lists, and
k_fast's values-only (REG) form against the ordinary kernel.

A row is regular when it has only 2-byte qualifiers, is neither malformed nor unsorted (within
the cell or against its series' earlier rows), and datapoint i sits at first + i * step seconds
with step >= 1 (a one-point row: step 1).  `reg_ref` below is the host reference: a plain walk
over the resident qualifier bytes, with ROW_ERR / ROW_UNSORTED taken from tests/index_ref.py.

Results of the REG form must equal the ordinary kernel's bit for bit (option REGULAR = 0 sends the
regular lists through it), and tsdbhip_debug_regular must show that REG tiles were launched.
"""
from __future__ import annotations

import struct

import numpy as np
import pytest

from opentsdb_amd import abi, synth
from opentsdb_amd import engine as E
from oracle import oracle as O
from tests import index_ref as R
from tests.index_ref import q2, q4
from tests.test_gpu_parity import assert_groups_match, T0
from tests.test_gpu_regroup import agg_name, dsq, identical, restricted
from tests.test_gpu_scale import assert_rows_equal

pytestmark = pytest.mark.gpu

H = 3600
PATHS = [("default", {}), ("unfused", dict(INDEX_FUSED=0)), ("generic", dict(INDEX_GENERIC=1))]
F32, F64 = 0xB, 0xF


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


# ---- cells -----------------------------------------------------------------------------------
def fcell(offs, vals, vl=4):
    """A cell of 2-byte qualifiers at second offsets `offs` with float values of vl bytes."""
    fl, fmt = (F32, ">f") if vl == 4 else (F64, ">d")
    q = b"".join(q2(int(o), fl) for o in offs)
    v = b"".join(struct.pack(fmt, float(x)) for x in vals) + (b"\x00" if len(offs) > 1 else b"")
    return q, v


def quarters(rng, n):
    """Multiples of 0.25 below 2^12: exact in float32, and every bucket sum passes the certificate."""
    return rng.integers(-(1 << 14), 1 << 14, n).astype(np.float64) * 0.25


def ap(first, step, n):
    return first + step * np.arange(n)


# ---- the host reference ----------------------------------------------------------------------
def reg_ref(host):
    """[rows, 2] {first, step} of the batch `host` (resident order), step 0 = not regular."""
    _, flags, _, _, _ = R.index_ref(host)
    qual = bytes(np.asarray(host.qual, np.uint8))
    qo = np.asarray(host.row_qual_off).astype(np.int64)
    out = np.zeros((len(flags), 2), np.uint32)
    for r in range(len(flags)):
        q = qual[qo[r]:qo[r + 1]]
        if flags[r] & (R.ROW_ERR | R.ROW_UNSORTED) or len(q) == 0 or len(q) % 2:
            continue
        offs, ok = [], True
        for i in range(0, len(q), 2):
            if (q[i] & 0xF0) == 0xF0:        # a 4-byte (millisecond) qualifier
                ok = False
                break
            offs.append(int.from_bytes(q[i:i + 2], "big") >> 4)
        if not ok:
            continue
        step = offs[1] - offs[0] if len(offs) > 1 else 1
        if step >= 1 and all(o == offs[0] + i * step for i, o in enumerate(offs)):
            out[r] = (offs[0], step)
    return out


def load_paths(eng, batch, ctx):
    """The batch on every load route: the side array against the reference, RowDesc fields equal
    across routes (the generic route is the one without any of the class kernels' marks)."""
    rows, regs = {}, {}
    ref = None
    for name, opts in PATHS:
        with E.options(**opts):
            eng.load(batch)
        rows[name] = tuple(a.copy() for a in eng.debug_rows())
        regs[name] = eng.debug_regular()[0].copy()
        if ref is None:
            ref = reg_ref(eng.download())
        np.testing.assert_array_equal(regs[name], ref, err_msg=f"{ctx} [{name}]: {{first, step}} vs the host walk")
    for name in ("default", "unfused"):   # (a malformed row's value statistics are never read)
        assert_rows_equal(rows[name], rows["generic"], f"{ctx}: RowDesc, {name} vs generic")
    return ref, rows["default"]


# ---- 1. index ----------------------------------------------------------------------------------
NPTS = [1, 2, 8, 9, 511, 512, 513, 1024, 1025]


def index_cases(rng):
    """[(name, cell, regular)] of one-row series."""
    cases = []

    def add(name, offs, regular, vl=4):
        cases.append((name, fcell(offs, quarters(rng, len(offs)), vl), regular))

    for n in NPTS:
        for step in (1, 7, 10, 60):
            if (n - 1) * step > 3599:
                continue
            for first in (0, 3599 - (n - 1) * step):       # first 0, and the last offset 3599
                add(f"n{n} step{step} first{first}", ap(first, step, n), True, 4 if (n + step) % 2 else 8)
    add("first 5 step 3", ap(5, 3, 700), True)
    for n, step in ((520, 2), (512, 3), (64, 10), (1030, 1)):
        full = ap(3, step, n + 1)
        for where, k in (("start", 1), ("chunk edge", 512), ("middle", n // 2)):
            if k >= n:
                continue
            add(f"n{n} step{step} missing at {where}", np.delete(full, k), False)
        rep = ap(3, step, n).copy()
        rep[n // 2] = rep[n // 2 - 1]
        add(f"n{n} step{step} repeated offset", rep, False)
        sw = ap(3, step, n).copy()
        sw[n // 3], sw[n // 3 + 1] = sw[n // 3 + 1], sw[n // 3]
        add(f"n{n} step{step} swapped pair", sw, False)
    add("missing second point of three", np.array([0, 2, 3]), False)
    add("last point late", np.append(ap(0, 5, 100), 3599), False)
    # evenly spaced, but the last offsets reach 0xF00: those qualifiers read as 4-byte ones
    add("offsets past 0xF00", ap(3500, 60, 8), False)
    add("offsets past 0xF00, long", ap(2000, 3, 640), False)
    # 4-byte (ms) qualifiers, regular in time all the same
    for n in (1, 9, 600):
        q = b"".join(q4(int(o) * 1000, F32) for o in ap(0, 5, n))
        v = b"".join(struct.pack(">f", x) for x in quarters(rng, n)) + (b"\x00" if n > 1 else b"")
        cases.append((f"ms qualifiers n{n}", (q, v), False))
    # mixed widths: one ms qualifier among seconds
    for n, k in ((9, 4), (600, 0), (600, 599)):
        offs = ap(0, 5, n)
        q = b"".join(q4(int(o) * 1000, F32) if i == k else q2(int(o), F32) for i, o in enumerate(offs))
        v = b"".join(struct.pack(">f", x) for x in quarters(rng, n)) + b"\x01"
        cases.append((f"mixed widths n{n} at {k}", (q, v), False))
    for name, q, v, bad in R.MALFORMED_CELLS:
        if bad and len(q):
            cases.append((f"malformed: {name}", (q, v), False))
    # regular offsets around a value the decoder refuses (a 3-byte float claim)
    offs = ap(0, 10, 20)
    q = b"".join(q2(int(o), 0xA if i == 7 else F32) for i, o in enumerate(offs))
    cases.append(("malformed value length in regular offsets", (q, b"\x00" * (19 * 4 + 3 + 1)), False))
    return cases


def test_index_regular_every_route(eng):
    rng = np.random.default_rng(5)
    cases = index_cases(rng)
    batch = R.one_row_batch([c for _, c, _ in cases], T0)
    ref, rows = load_paths(eng, batch, "index cases")
    # one-row series of one group each stay in batch order
    for (name, _, regular), (first, step) in zip(cases, ref):
        assert (step != 0) == regular, f"{name}: reference says {{first {first}, step {step}}}"
    assert sum(1 for *_, reg in cases if reg) > 40 and (rows[1] & R.ROW_ERR).any()


def test_index_regular_recede(eng):
    """A series whose second row starts before its first row ends: k_recede flags the second row
    unsorted and it loses its mark; its neighbours keep theirs."""
    rng = np.random.default_rng(6)

    def row(base, offs):
        q, v = fcell(offs, quarters(rng, len(offs)))
        return base, q, v

    series = [
        [row(T0, ap(0, 5, 720)), row(T0 + H, ap(0, 5, 720))],                 # in order
        [row(T0, ap(0, 3, 1000)), row(T0 + 1800, ap(0, 10, 100))],            # recedes: 2997 > 1800
        [row(T0, ap(0, 5, 300)), row(T0 + 1800, ap(0, 10, 100))],             # 1495 < 1800: in order
        [row(T0, ap(10, 1, 600)), row(T0 + 609, ap(0, 1, 600))],              # starts at the last datapoint before
        [row(T0, ap(10, 1, 600)), row(T0 + 610, ap(0, 1, 600))],              # ... and a second after it
    ]
    batch = synth.from_series(series, [0, 0, 1, 1, 2])
    ref, rows = load_paths(eng, batch, "recede")
    assert [int(s) for s in ref[:, 1]] == [5, 5, 3, 0, 5, 10, 1, 0, 1, 1]
    uns = (rows[1] & R.ROW_UNSORTED) != 0
    assert list(np.flatnonzero(uns)) == [3, 7]


# ---- stores for the query tests ---------------------------------------------------------------
def regular_store(n_series, n_groups, vl, seed, step=3, irregular=(), big=(), step2=None):
    """Two-hour series of two long rows each (600 .. 1100 points, regular); `irregular`: series
    whose second row misses a point; `big`: series holding one value that fails the certificate;
    step2: the second row's step (61: a 59-point row beside the long one, still the walker's tile)."""
    rng = np.random.default_rng(seed)
    series = []
    for s in range(n_series):
        rows = []
        for h in range(2):
            st = step2 if (h == 1 and step2) else step
            n = 600 + (s * 37 + h * 211) % 501
            n = min(n, 3599 // st + 1)
            offs = ap((s + h) % 5, st, n)
            offs = offs[offs <= 3599]
            if s in irregular and h == 1:
                offs = np.delete(offs, len(offs) // 2)
            vals = quarters(rng, len(offs))
            if s in big and h == 0:
                vals[len(vals) // 3] = float(2 ** 45)
            q, v = fcell(offs, vals, vl)
            rows.append((T0 + h * H, q, v))
        series.append(rows)
    return synth.from_series(series, [s % n_groups for s in range(n_series)])


def both(eng, run, ctx, expect_reg=True):
    """run() with the default options and with REGULAR = 0: bit-identical; the default one
    launched REG tiles, the other none.  Returns the default result."""
    got = run()
    launched = eng.debug_regular()[2]
    with E.options(REGULAR=0):
        base = run()
        assert eng.debug_regular()[2] == 0, f"{ctx}: REG tiles launched under REGULAR = 0"
    if expect_reg:
        assert launched > 0, f"{ctx}: no tile went through the REG form"
    pairs = zip(got, base) if isinstance(got, list) and got and isinstance(got[0], abi.Groups) else [(got, base)]
    for i, (g, b) in enumerate(pairs):
        identical(g, b, f"{ctx} [{i}] REG vs REGULAR = 0")
    return got


FAST_FNS = ["sum", "avg", "count", "min", "max", "squareSum"]


@pytest.fixture(scope="module", params=[(64, 4), (3, 4), (64, 8), (3, 8)], ids=lambda p: f"g{p[0]}-vl{p[1]}")
def store(request):
    g, vl = request.param
    return regular_store(131, g, vl, seed=100 + g + vl)


# ---- 2. query parity ----------------------------------------------------------------------------
def test_query_parity(eng, store):
    eng.load(store)
    fs, lists, _ = eng.debug_regular()
    assert (fs[:, 1] == 3).all() and int(lists.sum()) == store.n_series   # (one series a tile in a store this small)
    end = T0 + 2 * H

    def check(q, ctx, tol=None):
        got = both(eng, lambda: eng.run(q), ctx)
        assert_groups_match(got, O.run_query(store, q), agg_name(q), tol=tol, ctx=f"{ctx} vs oracle")

    for fn in FAST_FNS:                                   # KR 1: the plain group-by, K = 60
        check(dsq(T0, end, "sum", fn, 120000), f"sum:2m-{fn}")
    # KR 2: the fused multi-aggregator pass
    qs = [dsq(T0, end, a, "avg", 120000) for a in ("avg", "min", "max", "count", "dev")]
    multi = both(eng, lambda: eng.run_multi(qs), "run_multi")
    for q, g in zip(qs, multi):
        assert_groups_match(g, O.run_query(store, q), agg_name(q), ctx=f"run_multi {agg_name(q)} vs oracle")
    # KR 3: the per-series outputs -- p99 group-by, and an ordered sum
    check(dsq(T0, end, "p99", "avg", 120000), "p99:2m-avg", tol=0.0)
    check(dsq(T0, end, "sum", "sum", 120000, flags=abi.QF_ORDERED), "ordered sum:2m-sum")
    # KR 0: a rate query, and K > 64 (2 h of 1m buckets)
    check(dsq(T0, end, "sum", "avg", 120000, rate=True), "rate sum:2m-avg")
    check(dsq(T0, end, "sum", "avg", 60000), "sum:1m-avg K 120")


# ---- 3. edges of the fold -----------------------------------------------------------------------
@pytest.mark.parametrize("step", [7, 61, 1])
def test_fold_edges(eng, step):
    # (a row of step 61 has under 60 points: it rides in the walker's tile beside a long row;
    # a lane's 8 points then span 488 s, more than two 1m buckets)
    b = regular_store(70, 3, 4, seed=step, step=3, step2=61) if step == 61 else regular_store(70, 3, 4, seed=step, step=step)
    eng.load(b)
    assert int(eng.debug_regular()[1].sum()) == 70
    end = T0 + 2 * H
    cases = [("1m whole range", dsq(T0, end, "sum", "sum", 60000)),
             ("1m inside the rows", dsq(T0 + 1234, T0 + H + 2345, "sum", "avg", 60000)),     # n0 < 0 and slast >= K
             ("2m inside the first row", dsq(T0 + 601, T0 + 3001, "max", "max", 120000)),
             ("7s buckets inside a row", dsq(T0 + 1000, T0 + 1400, "sum", "min", 7000)),
             ("hour buckets", dsq(T0, end, "sum", "sum", 3600000)),                           # oneb
             ("hour buckets inside", dsq(T0 + 900, end - 900, "sum", "avg", 3600000)),
             ("two-hour bucket", dsq(T0, end, "sum", "count", 7200000))]
    for name, q in cases:
        got = both(eng, lambda: eng.run(q), f"step {step} {name}")
        assert_groups_match(got, O.run_query(b, q), agg_name(q), ctx=f"step {step} {name} vs oracle")


def test_certificate_hand_back(eng):
    """A series whose bucket sums cannot be certified: its tile goes from REG to k_grid."""
    b = regular_store(70, 3, 4, seed=9, step=1, big=(11, 40))
    eng.load(b)
    q = dsq(T0, T0 + 2 * H, "sum", "sum", 60000)
    got = both(eng, lambda: eng.run(q), "certificate")
    t = eng.timing()
    assert t.redo_tiles >= 2, "the uncertified series were not handed back"
    assert_groups_match(got, O.run_query(b, q), "sum", ctx="certificate vs oracle")


# ---- 4. mixed tiles -----------------------------------------------------------------------------
def test_mixed_tiles(eng):
    b = regular_store(70, 3, 4, seed=21, irregular=(17,))
    eng.load(b)
    fs, lists, _ = eng.debug_regular()
    ref = reg_ref(eng.download())
    np.testing.assert_array_equal(fs, ref)
    assert int((fs[:, 1] == 0).sum()) == 1
    eng.run(dsq(T0, T0 + 2 * H, "sum", "sum", 60000))
    t = eng.timing()
    # a store this small has one series a tile: the irregular row's tile stays on the ordinary list
    assert t.tiles == 70 and int(lists.sum()) == 69
    for fn in ("sum", "max"):
        q = dsq(T0, T0 + 2 * H, "sum", fn, 60000)
        got = both(eng, lambda: eng.run(q), f"mixed {fn}")
        assert_groups_match(got, O.run_query(b, q), "sum", ctx=f"mixed {fn} vs oracle")
    eng.run(dsq(T0, T0 + 2 * H, "sum", "sum", 60000))
    assert eng.debug_regular()[2] == 69


# ---- 5. append and regroup ----------------------------------------------------------------------
def reg_state(eng, queries):
    fs, lists, _ = eng.debug_regular()
    return [eng.run(q) for q in queries], fs.copy(), lists.copy(), tuple(a.copy() for a in eng.debug_rows())


def same_reg_state(a, b, ctx):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        identical(x, y, f"{ctx} q{i}")
    np.testing.assert_array_equal(a[1], b[1], err_msg=f"{ctx}: side array")
    np.testing.assert_array_equal(a[2], b[2], err_msg=f"{ctx}: regular lists")
    for x, y in zip(a[3], b[3]):
        np.testing.assert_array_equal(x, y, err_msg=f"{ctx}: RowDesc")


def test_append_and_regroup(eng):
    rng = np.random.default_rng(31)
    n = 40

    def row(h, step, n_pts, drop=None):
        offs = ap(1, step, n_pts)
        if drop is not None:
            offs = np.delete(offs, drop)
        q, v = fcell(offs, quarters(rng, len(offs)))
        return T0 + h * H, q, v

    first = [[row(0, 4, 800), row(1, 4, 700 + s)] for s in range(n)]
    # the delta: a third hour for every series -- regular, but irregular for series 5 and 22
    third = [[row(2, 5, 650 + s, drop=300 if s in (5, 22) else None)] for s in range(n)]
    gids = [s % 3 for s in range(n)]
    a = synth.from_series(first, gids)
    d = synth.from_series(third, gids)
    full = synth.from_series([x + y for x, y in zip(first, third)], gids)
    queries = [dsq(T0, T0 + 3 * H, "sum", "sum", 300000), dsq(T0, T0 + 3 * H, "max", "avg", 300000)]
    eng.load(a)
    assert int(eng.debug_regular()[1].sum()) == n
    eng.append(d, np.arange(n), np.zeros(n))
    got = reg_state(eng, queries)
    assert eng.debug_regular()[2] == n - 2
    np.testing.assert_array_equal(got[1], reg_ref(eng.download()))
    eng.load(full)
    same_reg_state(got, reg_state(eng, queries), "append vs fresh load")
    # regroup: the entries move with their rows
    ids = np.array([(s * 7) % 4 if s % 9 else abi.GROUP_EXCLUDED for s in range(n)], np.int32)
    eng.regroup(ids)
    got = reg_state(eng, queries)
    np.testing.assert_array_equal(got[1], reg_ref(eng.download()))
    rb, _ = restricted(full, ids)
    for q, g in zip(queries, got[0]):
        assert_groups_match(g, O.run_query(rb, q), agg_name(q), ctx="regroup vs oracle")
    eng.load(rb)
    same_reg_state(got, reg_state(eng, queries), "regroup vs fresh load")


# ---- 6. accounting ------------------------------------------------------------------------------
def test_accounting(eng):
    b = regular_store(70, 3, 4, seed=41)
    eng.load(b)
    nrows = b.n_rows
    qlen = int(b.row_qual_off[-1])
    vlen = int(b.row_val_off[-1])
    today = qlen + vlen + nrows * (4 + 16) + 4 * b.n_series
    q = dsq(T0, T0 + 2 * H, "sum", "avg", 60000)
    eng.run(q)
    assert eng.debug_regular()[2] == 70
    assert eng.timing().bytes == today - qlen + 8 * nrows
    with E.options(REGULAR=0):
        eng.run(q)
        assert eng.timing().bytes == today
    eng.run(q)
    assert eng.timing().bytes == today - qlen + 8 * nrows      # (the cache key holds what decides it)
    eng.run(dsq(T0, T0 + 2 * H, "none", "avg", 60000))
    assert eng.timing().bytes == today
    # one row's tile on the ordinary list: that row's qualifiers are read
    b2 = regular_store(70, 3, 4, seed=41, irregular=(17,))
    eng.load(b2)
    eng.run(q)
    qo = np.asarray(b2.row_qual_off).astype(np.int64)
    kept_q = int(qo[2 * 17 + 2] - qo[2 * 17])                   # series 17's two rows
    today2 = int(qo[-1]) + int(b2.row_val_off[-1]) + b2.n_rows * 20 + 4 * b2.n_series
    assert eng.timing().bytes == today2 - (int(qo[-1]) - kept_q) + 8 * (b2.n_rows - 2)
