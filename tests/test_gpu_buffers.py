"""The library's device and page-locked host buffers free themselves (csrc/devbuf.h): a closed engine
leaves none of them behind, whatever it ran, and a call repeated holds no more than the first one
did.  tsdbhip_debug_buffers counts the live buffers of the whole process, so every test reads its
`before` right before it opens an engine of its own: engines other tests hold do not matter."""
from __future__ import annotations

import numpy as np
import pytest

from opentsdb_amd import abi
from opentsdb_amd import engine as E
from opentsdb_amd.engine import Engine, EngineError
from tests import hist_util as U
from tests.put_util import store_batch
from tests.test_gpu_append import sizes
from tests.test_gpu_compaction import _random_scan
from tests.test_gpu_regroup import dsq, identical
from tests.test_put_cpu import PLACEMENTS

pytestmark = pytest.mark.gpu

T0 = 1356998400
H = 3600
N, G = 256, 8   # smoke()'s store: 256 series x 3600 points at 1 s, 8 groups


def points(groups):
    return sum(len(ts) for _, ts, _, _ in groups)


def test_destroy_frees_everything():
    before = E.debug_buffers()
    eng = Engine(0)
    try:
        # rows of at most 512 points, one a series (the short streaming tiles): what the sampled-window
        # select takes -- the 3600-point hour rows below never reach it
        eng.synth(N, T0, 360, 10000, 2, G, 30000, 0x5EED)
        r0 = eng.debug_sel_window()
        with E.options(SEL_WIN=2):
            assert len(eng.run(dsq(T0, T0 + H, "p99", "avg", 60000))) == G
        assert eng.debug_sel_window()[0] > r0[0], "the sampled-window select did not run"
        # two hour rows a series, so that a trim has rows to evict and rows to keep
        eng.synth(N, T0 + H // 2, 3600, 1000, 0, G, 1, 0x5EED)
        lo, hi = T0, T0 + 2 * H
        assert len(eng.run(dsq(lo, hi, "sum", "avg", 60000))) == G
        assert len(eng.run_multi([dsq(lo, hi, a, "avg", 60000) for a in ("sum", "min", "max")])) == 3
        assert points(eng.run(abi.new_query(T0 + H, T0 + H + 59, "sum"))) > 0, "the raw query returned nothing"
        iv = E.rollup_interval("10m", "1d")
        assert eng.rollup_run(iv, lo, hi)[0] > 0
        assert eng.preagg_run(iv, lo, hi, "sum")[0] > 0
        ids = np.arange(N, dtype=np.int32) % 4
        ids[::7] = abi.GROUP_EXCLUDED
        eng.regroup(ids)
        t = eng.trim(T0 + H, 0)
        assert t.rows_evicted > 0 and t.packed == 1, "the trim evicted nothing"
        info, _ = eng.remove([(1, T0 + H, T0 + 2 * H)])
        assert info.rows_removed > 0
        eng.load_tags(*abi.tag_table_arrays([[(2, 10 + s % 5), (3, 100 + s % 3)] for s in range(N)]))
        _, keys, tinfo = eng.regroup_tags([(3, abi.TF_IN, [100, 101])], group_by=[2])
        assert tinfo.n_groups == len(keys) == 5
        linfo = eng.last(anchor_s=T0 + H)[3]
        assert linfo.found > 0 and linfo.found + linfo.none == N
        held = E.debug_buffers()
        assert held.dev_n > before.dev_n and held.dev_bytes > before.dev_bytes, (before, held)
        assert held.host_n > before.host_n and held.host_bytes > before.host_bytes, (before, held)
    finally:
        eng.close()
    assert E.debug_buffers() == before


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def twice(call):
    """The counters after the first call and after the second."""
    call()
    first = E.debug_buffers()
    call()
    return first, E.debug_buffers()


def test_second_synth_holds_no_more(eng):
    first, second = twice(lambda: eng.synth(N, T0, 3600, 1000, 2, G, 1000, 7))   # (integers: the sizes pass's buffer too)
    assert second == first


def test_second_load_cells_holds_no_more(eng):
    series, groups = _random_scan(21)
    cb = abi.HostCellBatch.from_rows(series, groups, True)
    first, second = twice(lambda: eng.load_cells(cb))
    assert second == first


def test_second_load_tags_holds_no_more(eng):
    eng.synth(N, T0, 3600, 1000, 0, G, 1, 0x5EED)
    table = abi.tag_table_arrays([[(2, 10 + s % 5)] for s in range(N)])
    first, second = twice(lambda: eng.load_tags(*table))
    assert second == first


def test_second_refused_put_holds_no_more(eng):
    """A duplicate with other value bytes, without the fix flag, is refused on the device -- after the
    edit has allocated its grown blobs (option APPEND_RESERVE = 0: the load left no room)."""
    series_points, gids, puts = PLACEMENTS["equal_other_bytes"]
    q = dsq(T0, T0 + H, "sum", "sum", 60000)

    def refused():
        with pytest.raises(EngineError) as ei:
            eng.put(puts)
        assert ei.value.code == abi.TSDB_E_ILLEGAL_DATA

    with E.options(APPEND_RESERVE=0):
        eng.load(store_batch(series_points, gids))
        want = eng.run(q), sizes(eng)
        first, second = twice(refused)
    assert second == first
    identical(eng.run(q), want[0], "refused put")
    assert sizes(eng) == want[1]


def test_histogram_store_goes_with_the_engine():
    before = E.debug_buffers()
    e = Engine(0)
    try:
        hb = U.random_store(np.random.default_rng(17), n_series=7, n_rows=3, period_ms=10000, groups=3, layouts=3)
        e.load_histograms(hb)
        got = e.run_histogram(U.query(T0 + 600, T0 + 3 * H - 900, "sum", "1m-sum"), [50.0, 99.0], True)
        assert sum(len(g[0].ts) for g in got) > 0
        assert E.debug_buffers().dev_n > before.dev_n
    finally:
        e.close()
    assert E.debug_buffers() == before
