"""Host side of trimming the resident batch (tsdbhip_trim, query.ResidentSpans.trim): the
expectation builder trim_batch against stores built from full point lists, what
ResidentSpans.trim hands the engine and keeps, and the argument checks that need no device."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

from opentsdb_amd import abi, engine, synth
from opentsdb_amd.query import ResidentSpans
from tests.append_util import batches_equal, merge_batches, split
from tests.test_append_cpu import store_points
from tests.test_regroup_cpu import END, METRIC, START, FakeEngine, make_store, query
from tests.trim_util import aligned_scan, trim_batch

T0 = 1356998400
H = 3600
GIDS = [0, 1, -1, 0, abi.GROUP_EXCLUDED, 2]


@pytest.mark.parametrize("cutoff", [T0 - 1, T0, T0 + 1, T0 + H, T0 + H + 1700, T0 + 2 * H, T0 + 3 * H, T0 + 9 * H])
def test_trim_equals_the_store_from_the_first_kept_hour(cutoff):
    """Rows with base < cutoff go: what stays is the store's points from the first hour that
    starts at or after the cutoff, every series and id kept."""
    pts = store_points()
    full = synth.from_series([p.rows() for p in pts], GIDS)
    first_kept = -(-cutoff // H) * H
    want = synth.from_series([p.rows(first_kept, None) for p in pts], GIDS)
    got = trim_batch(full, cutoff)
    batches_equal(got, want)
    assert got.n_series == len(pts) and got.n_rows == len(pts) * max(0, min(3, (T0 + 3 * H - first_kept) // H))


def test_trims_compose_and_keep_empty_series():
    pts = store_points()
    pts[2] = type(pts[2])(pts[2].ts[:5], pts[2].lv[:5], pts[2].fv[:5], pts[2].kind[:5], pts[2].ms[:5])   # first hour only
    full = synth.from_series([p.rows() for p in pts], GIDS)
    for c1, c2 in ((T0 + H, T0 + 2 * H), (T0 + 2 * H, T0 + H), (T0 + H + 5, T0 + H), (0, T0 + H)):
        batches_equal(trim_batch(trim_batch(full, c1), c2), trim_batch(full, max(c1, c2)))
    t = trim_batch(full, T0 + H)
    assert t.n_series == full.n_series and t.group_id.tolist() == GIDS
    assert int(t.series_row_ptr[3] - t.series_row_ptr[2]) == 0


@pytest.mark.parametrize("cutoff", [T0 + H, T0 + 2 * H, T0 + H + 900])
def test_trim_commutes_with_a_later_delta(cutoff):
    """A delta whose rows all lie at or after the cutoff: trimming before or after the append
    gives the same batch (a series the delta skips included)."""
    pts = store_points()
    a, d, idx, new, full = split(pts, GIDS, T0 + 2 * H + 1500, delta=[True, True, False, True, True, True])
    assert int(d.row_base_time.min()) >= cutoff
    batches_equal(trim_batch(merge_batches(a, d, idx, new), cutoff), merge_batches(trim_batch(a, cutoff), d, idx, new))


def test_aligned_scan():
    assert aligned_scan([1, 16, 17, 0, 5]).tolist() == [0, 16, 32, 64, 64]


# ---- ResidentSpans.trim -------------------------------------------------------------------------
class TrimEngine(FakeEngine):
    def __init__(self):
        super().__init__()
        self.trims = []

    def trim(self, cutoff_s, pack_dead_pct=abi.TRIM_NO_PACK):
        self.trims.append((cutoff_s, pack_dead_pct))
        return abi.TrimInfo()


@pytest.mark.parametrize("new_start", [START + H, START + H + 1800, START + 3 * H])
def test_resident_spans_trim(new_start):
    st = make_store()
    fe = TrimEngine()
    rs = ResidentSpans(st, METRIC, START, END, engine=fe)
    keys = list(rs.span_keys)
    rs.trim(new_start)
    assert fe.trims == [(new_start, 50)]                 # the scan start is the cutoff; the default policy
    assert rs.scan_start_s == new_start and rs.scan_end_s == END
    assert rs.span_keys == keys                          # series indices keep their meaning
    fresh = dict(st.scan(METRIC, new_start, END))
    assert set(fresh) <= set(keys)
    emptied = [sk for sk in keys if sk not in fresh]
    assert len(emptied) == 1                             # the series with rows in the first hour only
    assert rs.spans == [(sk, fresh.get(sk, [])) for sk in keys]
    rs.trim(new_start, pack_dead_pct=abi.TRIM_NO_PACK)   # to the present start: legal, nothing goes
    assert fe.trims[-1] == (new_start, abi.TRIM_NO_PACK)
    assert rs.spans == [(sk, fresh.get(sk, [])) for sk in keys]


def test_resident_spans_trim_refusals():
    st = make_store()
    fe = TrimEngine()
    rs = ResidentSpans(st, METRIC, START + H, END, engine=fe)
    with pytest.raises(ValueError, match="cannot grow back"):
        rs.trim(START)
    with pytest.raises(ValueError, match="leaves it empty"):
        rs.trim(END)
    assert fe.trims == []
    rs.run(query(st, {"host": "*"}, start=START + H, end=END - 1))
    rs.trim(START + 2 * H)
    with pytest.raises(ValueError, match="outside the resident range"):
        rs.run(query(st, {"host": "*"}, start=START + H, end=END - 1))
    rs.run(query(st, {"host": "*"}, start=START + 2 * H, end=END - 1))


# ---- the C entry points without a device ----------------------------------------------------------
def test_export_and_illegal_arguments_need_no_device():
    assert "tsdbhip_trim" in engine.EXPORTS and "tsdbhip_debug_layout" in engine.EXPORTS
    L = engine.lib()
    info = abi.TrimInfo()
    IA = abi.TSDB_E_ILLEGAL_ARGUMENT
    assert L.tsdbhip_trim(None, 0, 0, C.byref(info)) == IA
    assert L.tsdbhip_trim(None, T0, abi.TRIM_NO_PACK, None) == IA
    assert L.tsdbhip_trim(None, T0, 101, None) == IA
    assert L.tsdbhip_debug_layout(None, None, None) == IA
    assert abi.TRIM_NO_PACK == -1
    assert L.tsdbhip_abi_version() == 12


def test_trim_info_matches_the_header():
    """abi.TrimInfo's fields, in order and by type, are the header's tsdbhip_trim_info."""
    import os
    hdr = open(os.path.join(os.path.dirname(engine.HERE), "include", "tsdbhip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} tsdbhip_trim_info;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    ctypes_of = {"int64_t": C.c_int64, "uint64_t": C.c_uint64, "int32_t": C.c_int32}
    assert [(n, ctypes_of[t]) for n, t in fields] == list(abi.TrimInfo._fields_)
    assert C.sizeof(abi.TrimInfo) == 80
    assert "#define TSDB_TRIM_NO_PACK (-1)" in hdr
