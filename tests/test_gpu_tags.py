"""GPU parity of tsdbhip_regroup_tags (k_tags.hip): tag filters, group keys and
their numbering on the device, against the plain-Python expectation of tests/tags_ref.py, which
never uses the engine.  Every case runs routed and under TAGS_SORT=1, with info.route asserted:
the route a call must take is worked out here from the code's own constants, read from the source.

State equivalence reuses tests/test_gpu_regroup.py: after regroup_tags(q) the context must be
the one regroup(ids of the expectation) leaves, so check_regroup's oracle and fresh-load parity run
over an engine whose regroup() is the tag call."""
from __future__ import annotations

import math
import os
import re
import struct

import numpy as np
import pytest

from opentsdb_amd import abi
from opentsdb_amd import engine as E
from tests import tags_ref as TR
from tests.test_gpu_append import batches_equal
from tests.test_gpu_preagg import MIX_END, MIX_START, mixed_store
from tests.test_gpu_regroup import MIX_IDS, check_regroup, dsq, identical, mix_queries

gpu = pytest.mark.gpu

T0 = 1356998400
EXCL, NONE = abi.GROUP_EXCLUDED, abi.GROUP_NONE
ANY, IN, NOT_IN, NOT_KEY = abi.TF_ANY, abi.TF_IN, abi.TF_NOT_IN, abi.TF_NOT_KEY
RANK, SORT, NOGROUP = abi.TAGS_ROUTE_RANK, abi.TAGS_ROUTE_SORT, abi.TAGS_ROUTE_NOGROUP
IA, IS, NI = abi.TSDB_E_ILLEGAL_ARGUMENT, abi.TSDB_E_ILLEGAL_STATE, abi.TSDB_E_NOT_IMPLEMENTED
WIDE = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]   # the unsigned-order trap


def constants():
    """The rank route's limits and the launch's block cap, from the source."""
    hdr = open(os.path.join(E.CSRC, "engine.h")).read()
    src = open(os.path.join(E.CSRC, "k_tags.hip")).read()
    uid = 1 << int(re.search(r"constexpr int64_t TAGS_RANK_UID_LIMIT = 1 << (\d+);", hdr).group(1))
    keys = 1 << int(re.search(r"constexpr int64_t TAGS_RANK_MAX_KEYS = 1 << (\d+);", hdr).group(1))
    block = int(re.search(r"constexpr int TAGS_BLOCK = (\d+);", src).group(1))
    cap = int(re.search(r"constexpr int64_t TAGS_MAX_BLOCKS = (\d+);", src).group(1))
    return uid, keys, block, cap


UID_LIMIT, MAX_KEYS, BLOCK, CAP = constants()


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def tiny_batch(n, base=T0, gid=NONE):
    """n series of one row with one one-byte integer datapoint each."""
    a = np.arange(n + 1, dtype=np.int64)
    return abi.HostBatch(a, np.full(n, base, np.uint32), a * 2, a, np.zeros(2 * n, np.uint8), np.ones(n, np.uint8),
                         np.full(n, gid, np.int32))


def load_rows(eng, rows):
    eng.load(tiny_batch(len(rows)))
    eng.load_tags(*abi.tag_table_arrays(rows))
    assert eng.tags_loaded() == (len(rows), sum(len(r) for r in rows))


def routed(rows, q, ids):
    """The route an unforced call must report."""
    _, group_by, _ = TR.parts(q)
    if not group_by:
        return NOGROUP
    if max((v for r in rows for _, v in r), default=0) >= UID_LIMIT:
        return SORT
    cards = [len({dict(r)[k] for r, i in zip(rows, ids) if i >= 0}) for k in group_by]
    return RANK if math.prod(cards) <= MAX_KEYS else SORT


def check_dry(eng, rows, q, ctx, want_route=None):
    """A dry run on both routes against the expectation: ids, keys, counters, route."""
    if not isinstance(q, abi.HostTagQuery):
        q = abi.HostTagQuery(*q)
    ids, keys = TR.group_ids(rows, q)
    route = routed(rows, q, ids)
    if want_route is not None:
        assert route == want_route, (ctx, route)
    for forced in (None, 1):
        with E.options(TAGS_SORT=forced):
            gi, gk, info = eng.regroup_tags(q, dry=True)
        c = f"{ctx} {'sort' if forced else 'routed'}"
        np.testing.assert_array_equal(gi, np.asarray(ids, np.int32), err_msg=c)
        assert gk == (keys if q.group_by_list else [()] * info.n_groups), c
        assert (info.visible, info.excluded, info.ungrouped, info.n_groups) == TR.counters(ids), c
        assert info.route == (route if not forced or route == NOGROUP else SORT), (c, info.route)
        assert info.regrouped == 0 and info.table_bytes == (len(rows) + 1) * 8 + sum(len(r) for r in rows) * 8, c
    return ids, keys


def random_rows(rng, n, pool, tagks=(2, 3, 5, 7, 11, 13, 17, 19)):
    """0, 1 and 8 tags among them; tagk 2 is the first of a series, 19 the last."""
    rows = []
    for i in range(n):
        k = [0, 1, 8][i % 3] if i < 6 else int(rng.integers(0, 9))
        ks = sorted(rng.choice(tagks, size=k, replace=False).tolist())
        rows.append([(int(t), int(pool[rng.integers(0, len(pool))])) for t in ks])
    return rows


def queries_for(pool):
    lo, hi = sorted(pool)[0], sorted(pool)[-1]
    some = sorted(set(pool[:3]))
    return [
        ([], [], False),                                             # no filter, no group-by
        ([(2, ANY, [])], [2], False),                                # the first tagk
        ([(19, ANY, [])], [19], False),                              # the last
        ([(3, IN, some)], [5], False),                               # a group-by tagk that no filter names
        ([(3, NOT_IN, some), (5, NOT_KEY, [])], [2, 19], False),
        ([(2, IN, [lo, hi]), (2, NOT_IN, [hi])], [], False),         # two filters on one tagk
        ([(7, IN, [])], [7], False),                                 # an empty set: every series excluded
        ([(7, NOT_IN, [])], [3, 7, 11], False),
        ([(2, ANY, []), (3, NOT_KEY, [])], [2], True),               # explicit_tags: exactly tagk 2
        ([(t, ANY, []) for t in (2, 3, 5, 7, 11, 13, 17, 19)], [2, 3, 5, 7, 11, 13, 17, 19], True),
    ]


# ---- dry runs ----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pool_name", ["small", "wide"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_dry_series_counts(eng, n, pool_name):
    rng = np.random.default_rng(n)
    pool = list(range(1, 9)) if pool_name == "small" else WIDE + [2, 0x80000001]
    rows = random_rows(rng, n, pool)
    load_rows(eng, rows)
    for i, q in enumerate(queries_for(pool)):
        check_dry(eng, rows, q, f"n={n} {pool_name} q{i}")


@gpu
def test_dry_more_series_than_the_grid_has_threads(eng):
    n = CAP * BLOCK + 1
    i = np.arange(n)
    rows = [[(1, int(a)), (2, int(b))] for a, b in zip(i % 1000 + 1, i)]
    load_rows(eng, rows)
    q = ([(1, IN, list(range(257, 323, 2))), (2, NOT_IN, [n - 1])], [1], False)   # a set of 33; the last series excluded
    ids, keys = check_dry(eng, rows, q, "grid cap", want_route=RANK)
    assert len(keys) == 33 and ids[n - 1] == EXCL and ids[n - 1 - 1000] >= 0


@gpu
@pytest.mark.parametrize("shape", ["G=1", "G=N", "first", "last", "cols1", "cols2", "cols3", "cols8"])
def test_dry_group_shapes(eng, shape):
    n = 130
    ks = list(range(1, 9))
    if shape == "G=1":
        rows, gb = [[(1, 4), (2, i)] for i in range(n)], [1]
    elif shape == "G=N":
        rows, gb = [[(1, (i * 37) % n)] for i in range(n)], [1]
    elif shape == "first":      # keys that differ only in the first column
        rows, gb = [[(1, i % 7), (2, 5), (3, 9)] for i in range(n)], [1, 2, 3]
    elif shape == "last":       # ... only in the last
        rows, gb = [[(1, 5), (2, 9), (3, i % 7)] for i in range(n)], [1, 2, 3]
    else:
        c = int(shape[4:])
        rows, gb = [[(k, (i * (k + 2)) % (2 + k % 3)) for k in ks] for i in range(n)], ks[:c]
    load_rows(eng, rows)
    ids, keys = check_dry(eng, rows, ([], gb, False), shape, want_route=RANK)
    assert len(keys) == {"G=1": 1, "G=N": n}.get(shape, len(keys)) and len(keys) >= 1


@gpu
def test_dry_unsigned_order(eng):
    """UIDs with the top bit set order after the small ones, in one column and in eight."""
    rows = [[(1, v)] for v in [0xFFFFFFFF, 0, 0x80000000, 1, 0x7FFFFFFF, 0x80000000, 0]]
    load_rows(eng, rows)
    ids, keys = check_dry(eng, rows, ([], [1], False), "one column", want_route=SORT)
    assert keys == [(0,), (1,), (0x7FFFFFFF,), (0x80000000,), (0xFFFFFFFF,)] and ids == [4, 0, 3, 1, 2, 3, 0]
    # eight columns of full 32-bit UIDs: a key of 256 bits
    rng = np.random.default_rng(3)
    rows = [[(k, WIDE[rng.integers(0, 5)]) for k in range(1, 9)] for _ in range(200)]
    rows += [list(r) for r in rows[:20]]   # repeated keys
    load_rows(eng, rows)
    ids, keys = check_dry(eng, rows, ([(1, NOT_IN, [1])], list(range(1, 9)), False), "eight columns", want_route=SORT)
    assert len(keys) > 100


@gpu
@pytest.mark.parametrize("size", [0, 1, 2, 33, 5000])
def test_dry_set_sizes(eng, size):
    """Values below the smallest entry, above the largest and between entries, for IN and NOT_IN."""
    entries = [10 + 4 * i for i in range(size)]
    probes = sorted({3, 9, 10, 11, 12, 14, 10 + 4 * (size // 2), 11 + 4 * (size // 2), 6 + 4 * size, 7 + 4 * size, 10 + 4 * size,
                     50000})
    rows = [[(1, v), (2, i)] for i, v in enumerate(probes)] + [[(2, 99)]]
    load_rows(eng, rows)
    for kind in (IN, NOT_IN):
        ids, _ = check_dry(eng, rows, ([(1, kind, entries)], [1], False), f"size {size} kind {kind}")
        for v, i in zip(probes, ids):
            assert (i != EXCL) == ((v in entries) == (kind == IN)), (size, kind, v)
        assert ids[-1] == (EXCL if kind == IN else NONE)   # the series without the tag


@gpu
def test_dry_every_kind_and_explicit_tags(eng):
    rows = [[(1, 5)], [(1, 6)], [(2, 5)], [], [(1, 5), (2, 1)], [(1, 5), (2, 1), (3, 2)], [(2, 1)]]
    load_rows(eng, rows)
    for kind, values in [(ANY, []), (IN, [5]), (IN, []), (NOT_IN, [5]), (NOT_IN, []), (NOT_KEY, [])]:
        check_dry(eng, rows, ([(1, kind, values)], [], False), f"kind {kind} {values}", want_route=NOGROUP)
    f = [(1, ANY, []), (2, IN, [1]), (7, NOT_KEY, [])]
    ids, _ = check_dry(eng, rows, (f, [], True), "explicit")
    assert ids == [EXCL, EXCL, EXCL, EXCL, 0, EXCL, EXCL]       # a missing, an exact and an extra tag
    ids, _ = check_dry(eng, rows, (f, [1, 2], False), "not explicit")
    assert ids == [EXCL, EXCL, EXCL, EXCL, 0, 0, EXCL]
    ids, keys = check_dry(eng, rows, ([], [], True), "explicit, no filter")   # only the tagless series
    assert ids == [EXCL, EXCL, EXCL, 0, EXCL, EXCL, EXCL] and keys == [()]
    ids, keys = check_dry(eng, rows, ([(9, ANY, [])], [1], False), "every series excluded")
    assert set(ids) == {EXCL} and keys == []
    ids, keys = check_dry(eng, rows, ([], [3], False), "a group-by tagk most series lack")
    assert ids == [NONE] * 5 + [0, NONE] and keys == [(2,)]


# ---- route edges -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("top,route", [(UID_LIMIT - 1, RANK), (UID_LIMIT, SORT)])
def test_route_edge_largest_uid(eng, top, route):
    rows = [[(1, [0, 31, 32, top - 1, top][i % 5]), (2, i % 3)] for i in range(65)]
    load_rows(eng, rows)
    ids, keys = check_dry(eng, rows, ([], [1, 2], False), f"top uid {top}", want_route=route)
    assert len(keys) == 15 and keys[-1] == (top, 2)


def factors_above(m):
    """a * b == m + 1 with both small, or the smallest square above m."""
    for a in range(int(math.isqrt(m + 1)), 1, -1):
        if (m + 1) % a == 0:
            return a, (m + 1) // a
    a = int(math.isqrt(m)) + 1
    return a, a


@gpu
@pytest.mark.parametrize("side", ["at", "above"])
def test_route_edge_composite_space(eng, side):
    if side == "at":
        a = 1 << (MAX_KEYS.bit_length() // 2)
        b = MAX_KEYS // a
        assert a * b == MAX_KEYS
    else:
        a, b = factors_above(MAX_KEYS)
        assert a * b > MAX_KEYS and max(a, b) < 1 << 17
    n = max(a, b)
    rows = [[(1, (i * 5 + 3) % a if n == a and math.gcd(5, a) == 1 else i % a), (2, i % b)] for i in range(n)]
    load_rows(eng, rows)
    ids, keys = TR.group_ids(rows, ([], [1, 2], False))
    assert len({k[0] for k in keys}) == a and len({k[1] for k in keys}) == b
    check_dry(eng, rows, ([], [1, 2], False), f"product {a} x {b}", want_route=RANK if side == "at" else SORT)


# ---- state equivalence -------------------------------------------------------------------------
def rows_for_ids(ids):
    """A tag table and a query whose answer is `ids` (dense group numbers): a unique host, the
    group as tagk 1, tagk 3 on the series to exclude."""
    rows = []
    for i, g in enumerate(ids):
        r = [(2, 500 + i)]
        if g >= 0:
            r.append((1, 10 + 3 * g))
        if g == EXCL:
            r.append((3, 99))
        rows.append(sorted(r))
    q = abi.HostTagQuery([(3, NOT_KEY, []), (2, ANY, [])], [1], False)
    assert TR.group_ids(rows, q)[0] == list(ids)
    return rows, q


class TagRegroup:
    """The engine with regroup(ids) answered by regroup_tags of a query that means those ids."""

    def __init__(self, eng, q, forced):
        self._eng, self._q, self._forced = eng, q, forced

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def load(self, batch):
        self._eng.load(batch)

    def regroup(self, ids):
        with E.options(TAGS_SORT=self._forced):
            got, keys, info = self._eng.regroup_tags(self._q)
        np.testing.assert_array_equal(got, np.asarray(ids, np.int32))
        assert info.regrouped == 1 and info.route == (SORT if self._forced else RANK)
        assert keys == [(10 + 3 * g,) for g in range(info.n_groups)]


@gpu
@pytest.mark.parametrize("forced", [None, 1], ids=["routed", "sort"])
def test_state_equals_regroup_by_ids(eng, forced):
    batch = mixed_store()
    rows, q = rows_for_ids(MIX_IDS)
    eng.load(batch)
    eng.load_tags(*abi.tag_table_arrays(rows))
    check_regroup(TagRegroup(eng, q, forced), batch, MIX_IDS, list(mix_queries().values()), f"tags {forced}", loaded=True)


@gpu
def test_download_equals_a_context_regrouped_by_ids(eng):
    batch = mixed_store()
    other = E.Engine(0)
    try:
        for ids in (MIX_IDS, [EXCL, 0, 0, NONE, 1, 1, EXCL, NONE, 0]):
            rows, q = rows_for_ids(ids)
            eng.load(batch)
            eng.load_tags(*abi.tag_table_arrays(rows))
            eng.regroup_tags(q)
            other.load(batch)
            other.regroup(ids)
            batches_equal(eng.download(), other.download())
            np.testing.assert_array_equal(eng.resident_groups(), other.resident_groups())
            assert eng.n_series() == other.n_series()
    finally:
        other.close()


def answers(eng):
    qs = [dsq(MIX_START, MIX_END, "sum", "avg", 600000), dsq(MIX_START, MIX_END, "none", "avg", 600000),
          abi.new_query(MIX_START, MIX_END - 1, "sum")]
    return [eng.run(q) for q in qs]


def same_state(a, b, ctx):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        identical(x, y, f"{ctx} q{i}")
    batches_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2], err_msg=ctx)
    assert a[3:] == b[3:], ctx


def state(eng):
    return answers(eng), eng.download(), eng.resident_groups(), eng.n_series(), eng.tags_loaded()


@gpu
def test_sequences_and_dry_runs(eng):
    batch = mixed_store()
    n = batch.n_series
    rows = [sorted([(2, 500 + i), (1, 10 + i % 3)] + ([(3, 7)] if i % 4 == 0 else [])) for i in range(n)]
    q1 = abi.HostTagQuery([(3, NOT_KEY, [])], [1])
    q2 = abi.HostTagQuery([(1, IN, [10, 12])], [2])
    eng.load(batch)
    eng.load_tags(*abi.tag_table_arrays(rows))
    eng.regroup_tags(q2)
    alone = state(eng)
    eng.load(batch)
    eng.load_tags(*abi.tag_table_arrays(rows))
    ids1, keys1, _ = eng.regroup_tags(q1)
    first = state(eng)
    eng.regroup(MIX_IDS)
    ids2, keys2, _ = eng.regroup_tags(q2)
    same_state(state(eng), alone, "regroup_tags / regroup / regroup_tags")
    assert keys2 == TR.group_ids(rows, q2)[1] and list(ids2) == TR.group_ids(rows, q2)[0]
    # a dry run between two queries changes no answer, and reports the other query's ids and keys
    eng.regroup_tags(q1)
    same_state(state(eng), first, "q1 again")
    dry_ids, dry_keys, info = eng.regroup_tags(q2, dry=True)
    assert info.regrouped == 0 and dry_keys == keys2
    np.testing.assert_array_equal(dry_ids, ids2)
    same_state(state(eng), first, "after a dry run")
    eng.regroup_tags(q2)
    same_state(state(eng), alone, "q2 after the dry run")


# ---- lifetime of the table -----------------------------------------------------------------------
@gpu
def test_table_lifetime(eng):
    n = 6
    rows = [[(1, i % 2), (2, i)] for i in range(n)]
    q = abi.HostTagQuery([], [1])

    def fresh():
        eng.load(tiny_batch(n))
        eng.load_tags(*abi.tag_table_arrays(rows))

    def gone():
        assert eng.tags_loaded() == (0, 0)
        with pytest.raises(E.EngineError) as x:
            eng.regroup_tags(q)
        assert x.value.code == IS

    assert E.Engine is not None
    fresh()
    want = TR.group_ids(rows, q)[0]
    eng.trim(T0)
    eng.put([(0, T0 + 5, abi.PUT_LONG, 7)])
    eng.last(None, T0)
    eng.upsert(tiny_batch(1, base=T0 + 3600, gid=EXCL), [2], [0])   # a new row of a resident series
    eng.regroup([0, 1, EXCL, NONE, 0, 1])
    assert eng.tags_loaded() == (n, 2 * n)
    assert list(eng.regroup_tags(q)[0]) == want
    eng.load(tiny_batch(n))
    gone()
    fresh()
    eng.upsert(tiny_batch(1, base=T0 + 3600, gid=EXCL), [n], [1])   # a new series
    gone()
    fresh()
    eng.remove([(1, T0, T0 + 1)], drop_empty=True)                  # a retired series
    gone()
    fresh()
    eng.remove([(1, T0, T0 + 1)], drop_empty=False)                 # emptied, not retired: the numbering stays
    assert eng.tags_loaded() == (n, 2 * n) and list(eng.regroup_tags(q)[0]) == want


# ---- refusals ---------------------------------------------------------------------------------------
def raw_query(filters=(), sets=(), group_by=(), explicit=0, n_filters=None, n_set=None, n_group_by=None):
    """A tsdbhip_tag_query with every field as given, ranges unchecked."""
    fa = (abi.TagFilter * max(1, len(filters)))(*[abi.TagFilter(*f) for f in filters])
    sa = np.asarray(list(sets) or [0], np.uint32)
    ga = np.asarray(list(group_by) or [0], np.uint32)
    q = abi.TagQuery(len(filters) if n_filters is None else n_filters, C_void(fa), len(sets) if n_set is None else n_set,
                     sa.ctypes.data, len(group_by) if n_group_by is None else n_group_by, ga.ctypes.data, explicit)
    return q, (fa, sa, ga)


def C_void(arr):
    import ctypes as C
    return C.cast(arr, C.c_void_p)


def last_keys(eng, n):
    """The keys of the last call that succeeded, n words of them."""
    kw = np.full(n + 2, 0xDEAD, np.uint32)
    assert E.lib().tsdbhip_tags_keys(eng.ctx, kw.ctypes.data) == 0
    assert kw[n] == kw[n + 1] == 0xDEAD
    return kw[:n].tolist()


def tags_code(eng, q, flags=0):
    import ctypes as C
    return E.lib().tsdbhip_regroup_tags(eng.ctx, C.byref(q[0]) if q is not None else None, flags, None, None)


def table_code(eng, n, ptr, tagk, tagv):
    import ctypes as C
    ptr, tagk, tagv = (None if a is None else np.ascontiguousarray(a, d) for a, d in ((ptr, np.int64), (tagk, np.uint32), (tagv, np.uint32)))
    t = abi.TagTable(n, None if ptr is None else ptr.ctypes.data, None if tagk is None else tagk.ctypes.data,
                     None if tagv is None else tagv.ctypes.data)
    return E.lib().tsdbhip_tags_load(eng.ctx, C.byref(t))


@gpu
def test_refusals_leave_everything(eng):
    import ctypes as C
    batch = mixed_store()
    n = batch.n_series
    rows, q = rows_for_ids(MIX_IDS)
    eng.load(batch)
    # without a table, without a previous call
    assert tags_code(eng, (q.c,)) == IS
    assert E.lib().tsdbhip_tags_keys(eng.ctx, None) == IS
    eng.load_tags(*abi.tag_table_arrays(rows))
    assert E.lib().tsdbhip_tags_keys(eng.ctx, None) == IS
    eng.regroup_tags(q)
    before = state(eng)
    keys_before = last_keys(eng, 4)
    assert keys_before == [10, 13, 16, 19]
    ptr, tk, tv = abi.tag_table_arrays(rows)
    bad_ptr = ptr.copy()
    bad_ptr[3], bad_ptr[4] = ptr[4], ptr[3]
    from1 = ptr.copy()
    from1[0] = 1
    dup = tk.copy()
    dup[ptr[0] + 1] = dup[ptr[0]]   # series 0 has two tags: the second no longer above the first
    for ctx, code in [
        ("null table", E.lib().tsdbhip_tags_load(eng.ctx, None)),
        ("null tag_ptr", table_code(eng, n, None, tk, tv)),
        ("null tagk", table_code(eng, n, ptr, None, tv)),
        ("n_series short", table_code(eng, n - 1, ptr[:-1], tk, tv)),
        ("n_series long", table_code(eng, n + 1, np.append(ptr, ptr[-1]), tk, tv)),
        ("tag_ptr not from 0", table_code(eng, n, from1, tk, tv)),
        ("tag_ptr descending", table_code(eng, n, bad_ptr, tk, tv)),
        ("tagks not ascending", table_code(eng, n, ptr, dup, tv)),
        ("null query", tags_code(eng, None)),
        ("unknown flag", tags_code(eng, (q.c,), flags=2)),
        ("unknown kind", tags_code(eng, raw_query([(1, 4, 0, 0)]))),
        ("negative kind", tags_code(eng, raw_query([(1, -1, 0, 0)]))),
        ("set past n_set", tags_code(eng, raw_query([(1, IN, 0, 3)], sets=[1, 2]))),
        ("set before 0", tags_code(eng, raw_query([(1, IN, -1, 1)], sets=[1, 2]))),
        ("set backwards", tags_code(eng, raw_query([(1, IN, 2, 1)], sets=[1, 2]))),
        ("set not ascending", tags_code(eng, raw_query([(1, IN, 0, 3)], sets=[1, 3, 3]))),
        ("group_by not ascending", tags_code(eng, raw_query(group_by=[2, 2]))),
        ("group_by descending", tags_code(eng, raw_query(group_by=[2, 1]))),
        ("nine group-bys", tags_code(eng, raw_query(group_by=list(range(1, 10))))),
        ("65 filters", tags_code(eng, raw_query([(1, ANY, 0, 0)] * 65))),
        ("negative n_filters", tags_code(eng, raw_query(n_filters=-1))),
        ("explicit_tags 2", tags_code(eng, raw_query(explicit=2))),
        ("null filters", E.lib().tsdbhip_regroup_tags(eng.ctx, C.byref(abi.TagQuery(1, None, 0, None, 0, None, 0)), 0, None, None)),
        ("null set", E.lib().tsdbhip_regroup_tags(eng.ctx, C.byref(abi.TagQuery(0, None, 1, None, 0, None, 0)), 0, None, None)),
        ("null group_by", E.lib().tsdbhip_regroup_tags(eng.ctx, C.byref(abi.TagQuery(0, None, 0, None, 1, None, 0)), 0, None, None)),
    ]:
        assert code == IA, ctx
        same_state(state(eng), before, ctx)
        assert last_keys(eng, 4) == keys_before, ctx
    # the limits themselves are legal
    assert tags_code(eng, raw_query([(1, ANY, 0, 0)] * 64, group_by=list(range(1, 9))), flags=abi.TAGS_DRY) == 0
    assert eng.regroup_tags(q, dry=True)[1] == [(k,) for k in keys_before]


@gpu
def test_not_implemented(eng):
    from opentsdb_amd.rollup_read import make_rollup_batch
    iv = E.rollup_interval("10m", "1d")
    cell = (struct.pack(">H", (0 << 4) | 0x7), struct.pack(">q", 5))
    q = abi.HostTagQuery([], [1])
    eng.load_rollup(make_rollup_batch([(None, [(T0, [cell], [])])], [0], iv, False))
    assert table_code(eng, 1, [0, 1], [1], [1]) == NI and tags_code(eng, (q.c,)) == NI
    assert "rollup batch" in E.lib().tsdbhip_last_error().decode()
    batch = mixed_store()
    n = batch.n_series
    rows, _ = rows_for_ids(MIX_IDS)
    eng.load_shard(batch, E.SHARD_SPANS, 0, n)
    assert table_code(eng, n, *abi.tag_table_arrays(rows)) == NI and tags_code(eng, (q.c,)) == NI
    assert "a shard's groups are numbered globally" in E.lib().tsdbhip_last_error().decode()
    assert eng.tags_loaded() == (0, 0)
    md = E.Engine(devices=[0, 0])
    try:
        md.load(batch)
        assert table_code(md, n, *abi.tag_table_arrays(rows)) == NI and tags_code(md, (q.c,)) == NI
        assert "multi-device context" in E.lib().tsdbhip_last_error().decode()
        assert E.lib().tsdbhip_tags_keys(md.ctx, None) == NI
    finally:
        md.close()
    eng.load(batch)
    eng.load_tags(*abi.tag_table_arrays(rows))   # and a whole load takes a table
    assert eng.tags_loaded()[0] == n


# ---- ResidentSpans end to end -----------------------------------------------------------------------
@gpu
def test_resident_spans_device_tags_equal_host_path(eng):
    from opentsdb_amd.query import ResidentSpans
    from tests.test_tags_cpu import END, METRIC, START, query, random_store
    store = random_store(21, n=60)
    forms = [({"dc": "*"}, [], False), ({"host": "h01|h02|h03", "dc": "*"}, [], False), ({"rack": "*", "dc": "lga"}, [], False),
             ({}, [], False), ({"dc": "nowhere"}, [], False)]
    for t, f in [("literal_or", "lga|sjc"), ("iliteral_or", "Lga"), ("not_literal_or", "lga"), ("not_iliteral_or", "lga"),
                 ("wildcard", "l*"), ("iwildcard", "L*a"), ("regexp", "^(lga|ams)$")]:
        forms.append(({}, [{"type": t, "tagk": "dc", "filter": f, "groupBy": True}], False))
        forms.append(({"host": "*"}, [{"type": t, "tagk": "dc", "filter": f}], True))
    forms.append(({"host": "*"}, [{"type": "not_key", "tagk": "rack", "filter": ""}], False))
    forms.append(({"host": "*", "dc": "*"}, [{"type": "not_key", "tagk": "rack", "filter": ""}], True))
    want = []
    for tags, filters, explicit in forms:
        q = query(store, tags, filters, explicit)
        q.downsample("10m-avg")
        q.runner = eng.run_batch
        want.append(q.run())
    assert sum(1 for w in want if w) >= len(forms) // 2
    for device_tags in (False, True):
        rs = ResidentSpans(store, METRIC, START, END, engine=eng, device_tags=device_tags)
        for (tags, filters, explicit), exp in zip(forms, want):
            q = query(store, tags, filters, explicit)
            q.downsample("10m-avg")
            got = rs.run(q)
            assert len(got) == len(exp), (device_tags, tags, filters)
            assert len({d.group_key for d in exp}) == len(exp)
            by = {d.group_key: d for d in got}
            for d in exp:
                g = by[d.group_key]
                for name in ("ts", "bits", "is_int"):
                    np.testing.assert_array_equal(getattr(g, name), getattr(d, name), err_msg=f"{device_tags} {tags} {filters} {name}")
