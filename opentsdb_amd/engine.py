"""ctypes binding of libtsdbhip (the MI355X engine behind include/tsdbhip.h).

The shared library is built in-tree (opentsdb_amd/lib/libtsdbhip.so, see
opentsdb_amd/csrc/Makefile).  There is no CPU fallback: if the library or a HIP device
is missing, constructing an Engine raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import time

import numpy as np

from . import abi
from . import histogram as H

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TSDBHIP_LIB") or os.path.join(HERE, "lib", "libtsdbhip.so")
CSRC = os.path.join(HERE, "csrc")

# every symbol include/tsdbhip.h declares
EXPORTS = [
    "tsdbhip_abi_version", "tsdbhip_last_error", "tsdbhip_aggregator_get", "tsdbhip_aggregator_interpolation",
    "tsdbhip_parse_duration", "tsdbhip_parse_downsample", "tsdbhip_scan_bounds", "tsdbhip_init",
    "tsdbhip_destroy", "tsdbhip_load", "tsdbhip_synth", "tsdbhip_batch_sizes", "tsdbhip_batch_download",
    "tsdbhip_run", "tsdbhip_result_free", "tsdbhip_last_timing", "tsdbhip_partials_layout_get",
    "tsdbhip_run_partials", "tsdbhip_run_partials_multi", "tsdbhip_finalize", "tsdbhip_sync", "tsdbhip_rollup_interval_parse",
    "tsdbhip_rollup_basetime", "tsdbhip_rollup_qualifier", "tsdbhip_rollup_run", "tsdbhip_rollup_download",
    "tsdbhip_sel_layout", "tsdbhip_sel_run_values", "tsdbhip_sel_select", "tsdbhip_assemble", "tsdbhip_run_multi",
    "tsdbhip_debug_rows", "tsdbhip_debug_index", "tsdbhip_debug_sel_window", "tsdbhip_shard_bounds", "tsdbhip_load_shard", "tsdbhip_synth_shard",
    "tsdbhip_load_rollup", "tsdbhip_load_cells", "tsdbhip_load_histograms", "tsdbhip_hist_run",
    "tsdbhip_hist_run_range", "tsdbhip_hist_result_free", "tsdbhip_expr_map", "tsdbhip_expr_zip", "tsdbhip_expr_topn",
    "tsdbhip_batch_range_sizes", "tsdbhip_batch_download_range", "tsdbhip_expr_sync", "tsdbhip_init_devices",
    "tsdbhip_md_shard_mode", "tsdbhip_md_info", "tsdbhip_host_alloc", "tsdbhip_host_free", "tsdbhip_md_stats",
    "tsdbhip_device_count", "tsdbhip_set_option", "tsdbhip_get_option", "tsdbhip_preagg_run", "tsdbhip_preagg_download",
    "tsdbhip_regroup", "tsdbhip_append", "tsdbhip_debug_regular", "tsdbhip_trim", "tsdbhip_debug_layout",
    "tsdbhip_debug_loaded", "tsdbhip_upsert", "tsdbhip_debug_rollup", "tsdbhip_debug_pct", "tsdbhip_debug_buffers",
    "tsdbhip_remove", "tsdbhip_last", "tsdbhip_put",
    "tsdbhip_tags_load", "tsdbhip_tags_loaded", "tsdbhip_regroup_tags", "tsdbhip_tags_keys",
]

# developer options (tsdbhip_set_option, opentsdb_amd/csrc/opts.h)
OPTIONS = ["FAST", "SHORT", "ROWS", "HWIN", "SEQ", "SEQ_ROWS", "SEQ_WAVE", "INDEX_GENERIC", "INDEX_FUSED", "CMP_CHUNK", "CMP_ROWS",
           "CMP_ONEPASS", "PCT_ROWS", "PCT_KEYS", "PCT_VONLY", "PCT_V6", "SEL_FUSED", "SEL_COLS", "SEL_WIN", "SEL_WAVE",
           "SEL_REG", "SELOPS", "RAW_LERPW", "RAW_SEL_TOP", "RAW_SEL_REG", "RO_FUSE", "RO_RUNS", "MULTI_FUSE", "EMIT_HALF", "HIST_WINDOW",
           "HIST_WS", "HIST_LAYOUT", "APPEND_RESERVE", "REGULAR", "LAST_WALK", "PUT_WALK", "TAGS_SORT", "TRACE", "DBG"]

IDX_C_SHORT4, IDX_C_SHORTV, IDX_C_FAIL = 12, 13, 14                # engine.h: tsdbhip_debug_index slots
SHARD_AUTO, SHARD_SERIES, SHARD_GROUPS, SHARD_SPANS = -1, 0, 1, 2   # tsdbhip.h TSDB_SHARD_*
MD_AUTO, MD_COPY, MD_RCCL = -1, 0, 1                               # tsdbhip.h TSDB_MD_*


class _PinnedBlock:
    """Page-locked host memory (tsdbhip_host_alloc) exposed through __array_interface__: numpy
    arrays over it keep this object as their base (views collapse to it), so the block is freed
    only when the last array over it is gone."""

    def __init__(self, nbytes: int, dtype, shape):
        p = C.c_void_p()
        _check(lib().tsdbhip_host_alloc(max(1, int(nbytes)), C.byref(p)))
        self.ptr = p.value
        self.__array_interface__ = {"data": (self.ptr, False), "shape": tuple(shape),
                                    "typestr": np.dtype(dtype).str, "version": 3}

    def __del__(self):
        if getattr(self, "ptr", None) and _lib is not None:
            _lib.tsdbhip_host_free(self.ptr)
            self.ptr = None


def pinned_copy(a: np.ndarray) -> np.ndarray:
    """`a` copied into page-locked host memory (uploads from it are DMA transfers)."""
    a = np.ascontiguousarray(a)
    out = np.asarray(_PinnedBlock(a.nbytes, a.dtype, a.shape))
    out[...] = a
    return out


class EngineError(Exception):
    def __init__(self, code: int, msg: str):
        self.code = code
        self.java = abi.ERROR_NAMES.get(code, str(code))
        super().__init__(f"{self.java}: {msg}")


def build(force: bool = False) -> str:
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-j8", "-C", CSRC], check=True)
    return LIB_PATH


_lib = None


def lib():
    """Loads libtsdbhip.so (fails loudly if it is not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"libtsdbhip is not built ({LIB_PATH}); run `make -C {CSRC}`")
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.tsdbhip_last_error.restype = C.c_char_p
        L.tsdbhip_aggregator_get.argtypes = [C.c_char_p]
        L.tsdbhip_parse_duration.argtypes = [C.c_char_p, C.POINTER(C.c_int64)]
        L.tsdbhip_parse_downsample.argtypes = [C.c_char_p, C.POINTER(abi.Query)]
        L.tsdbhip_scan_bounds.argtypes = [C.POINTER(abi.Query), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.tsdbhip_init.argtypes = [C.c_int, C.POINTER(vp)]
        L.tsdbhip_init_devices.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(vp)]
        L.tsdbhip_md_shard_mode.argtypes = [vp, C.c_int]
        L.tsdbhip_md_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]
        L.tsdbhip_device_count.argtypes = [C.POINTER(C.c_int)]
        L.tsdbhip_set_option.argtypes = [C.c_char_p, C.c_int64]
        L.tsdbhip_get_option.argtypes = [C.c_char_p, C.POINTER(C.c_int64)]
        L.tsdbhip_md_stats.argtypes = [vp, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.tsdbhip_destroy.argtypes = [vp]
        L.tsdbhip_host_alloc.argtypes = [C.c_uint64, C.POINTER(vp)]
        L.tsdbhip_host_free.argtypes = [vp]
        L.tsdbhip_host_free.restype = None
        L.tsdbhip_load.argtypes = [vp, C.POINTER(abi.Batch)]
        L.tsdbhip_regroup.argtypes = [vp, C.c_void_p, C.c_int64]
        L.tsdbhip_append.argtypes = [vp, C.POINTER(abi.Batch), C.c_void_p, C.c_void_p, C.POINTER(abi.AppendInfo)]
        L.tsdbhip_upsert.argtypes = [vp, C.POINTER(abi.Batch), C.c_void_p, C.c_void_p, C.POINTER(abi.UpsertInfo)]
        L.tsdbhip_trim.argtypes =[vp, C.c_int64, C.c_int32, C.POINTER(abi.TrimInfo)]
        L.tsdbhip_remove.argtypes = [vp, vp, C.c_int64, C.c_uint32, C.c_int32, vp, C.POINTER(abi.RemoveInfo)]
        L.tsdbhip_last.argtypes = [vp, vp, C.c_int64, C.c_int64, vp, C.c_int32, vp, vp, vp, C.POINTER(abi.LastInfo)]
        L.tsdbhip_put.argtypes = [vp, vp, C.c_int64, C.c_uint32, C.POINTER(abi.PutInfo)]
        L.tsdbhip_tags_load.argtypes = [vp, C.POINTER(abi.TagTable)]
        L.tsdbhip_tags_loaded.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.tsdbhip_regroup_tags.argtypes = [vp, C.POINTER(abi.TagQuery), C.c_uint32, vp, C.POINTER(abi.TagsInfo)]
        L.tsdbhip_tags_keys.argtypes = [vp, vp]
        L.tsdbhip_debug_layout.argtypes = [vp, C.c_void_p, C.c_void_p]
        L.tsdbhip_debug_loaded.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.tsdbhip_synth.argtypes = [vp, C.POINTER(abi.SynthSpec)]
        L.tsdbhip_batch_sizes.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64)]
        L.tsdbhip_batch_download.argtypes = [vp] + [C.c_void_p] * 7
        L.tsdbhip_batch_range_sizes.argtypes = [vp, C.c_int64, C.c_int64, C.POINTER(C.c_int64),
                                                C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.tsdbhip_batch_download_range.argtypes = [vp, C.c_int64, C.c_int64] + [C.c_void_p] * 7
        L.tsdbhip_run.argtypes = [vp, C.POINTER(abi.Query), C.POINTER(C.POINTER(abi.Result))]
        L.tsdbhip_result_free.argtypes = [C.POINTER(abi.Result)]
        L.tsdbhip_last_timing.argtypes = [vp, C.POINTER(abi.Timing)]
        L.tsdbhip_partials_layout_get.argtypes = [vp, C.POINTER(abi.Query), C.c_int64, C.POINTER(abi.PartialsLayout)]
        L.tsdbhip_run_partials.argtypes = [vp, C.POINTER(abi.Query), C.c_int64, C.c_void_p]
        L.tsdbhip_run_partials_multi.argtypes = [vp, C.POINTER(abi.Query), C.c_int, C.c_int64, C.c_void_p]
        L.tsdbhip_finalize.argtypes = [vp, C.POINTER(abi.Query), C.c_int64, C.c_void_p, C.c_int,
                                       C.POINTER(C.POINTER(abi.Result))]
        L.tsdbhip_sync.argtypes = [vp]
        L.tsdbhip_run_multi.argtypes = [vp, C.POINTER(abi.Query), C.c_int, C.POINTER(C.POINTER(abi.Result))]
        L.tsdbhip_sel_layout.argtypes = [vp, C.POINTER(abi.Query), C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]
        L.tsdbhip_sel_run_values.argtypes = [vp, C.POINTER(abi.Query), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tsdbhip_sel_select.argtypes = [vp, C.POINTER(abi.Query), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]
        L.tsdbhip_assemble.argtypes = [vp, C.POINTER(abi.Query), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(C.POINTER(abi.Result))]
        L.tsdbhip_rollup_interval_parse.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(abi.RollupInterval)]
        L.tsdbhip_rollup_basetime.argtypes = [C.c_int64, C.POINTER(abi.RollupInterval), C.POINTER(C.c_int32)]
        L.tsdbhip_rollup_qualifier.argtypes = [C.c_int64, C.c_int32, C.c_int16, C.c_int32,
                                               C.POINTER(abi.RollupInterval), C.c_void_p]
        L.tsdbhip_rollup_run.argtypes = [vp, C.POINTER(abi.RollupSpec), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
        L.tsdbhip_rollup_download.argtypes = [vp] + [C.c_void_p] * 5
        L.tsdbhip_preagg_run.argtypes = [vp, C.POINTER(abi.PreaggSpec), C.POINTER(C.c_int64), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64)]
        L.tsdbhip_preagg_download.argtypes = [vp] + [C.c_void_p] * 7
        L.tsdbhip_debug_rows.argtypes = [vp] + [C.c_void_p] * 4
        L.tsdbhip_debug_regular.argtypes = [vp, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.tsdbhip_debug_index.argtypes = [vp, C.c_void_p, C.POINTER(C.c_int)]
        L.tsdbhip_debug_sel_window.argtypes = [vp, C.c_void_p, C.c_void_p]
        L.tsdbhip_debug_rollup.argtypes = [vp, C.c_void_p]
        L.tsdbhip_debug_pct.argtypes = [vp, C.c_void_p]
        L.tsdbhip_debug_buffers.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_uint64)] * 2
        L.tsdbhip_shard_bounds.argtypes = [C.POINTER(abi.Batch), C.c_int, C.c_int, C.c_void_p]
        L.tsdbhip_load_shard.argtypes = [vp, C.POINTER(abi.Batch), C.c_int, C.c_int64, C.c_int64]
        L.tsdbhip_synth_shard.argtypes = [vp, C.POINTER(abi.SynthSpec), C.c_int64, C.c_int64]
        L.tsdbhip_load_rollup.argtypes = [vp, C.POINTER(abi.RollupBatch)]
        L.tsdbhip_load_cells.argtypes = [vp, C.POINTER(abi.CellBatch)]
        L.tsdbhip_load_histograms.argtypes = [vp, C.POINTER(H.HistBatch)]
        L.tsdbhip_hist_run.argtypes = [vp, C.POINTER(abi.Query), C.c_int, C.POINTER(C.c_float), C.c_int,
                                       C.POINTER(C.POINTER(H.HistResult))]
        L.tsdbhip_hist_run_range.argtypes = [vp, C.POINTER(abi.Query), C.c_int64, C.c_int64, C.c_int,
                                             C.POINTER(C.c_float), C.c_int, C.POINTER(C.POINTER(H.HistResult))]
        L.tsdbhip_hist_result_free.argtypes = [C.POINTER(H.HistResult)]
        _lib = L
    return _lib


def _check(rc):
    if rc < 0:
        raise EngineError(rc, lib().tsdbhip_last_error().decode(errors="replace"))
    return rc


def device_count() -> int:
    """HIP devices visible to the library (tsdbhip_device_count).  Use this rather than
    torch.cuda.device_count() before building an RCCL context: torch's wheel carries its own
    HIP / HSA runtime, and initialising it beside the library's broke ncclCommInitAll here."""
    n = C.c_int()
    _check(lib().tsdbhip_device_count(C.byref(n)))
    return n.value


def set_option(name: str, value) -> None:
    """tsdbhip_set_option: a developer option (kernel choice for tests / A/B runs), process-wide;
    None or -1 resets it to the production choice."""
    _check(lib().tsdbhip_set_option(name.encode(), -1 if value is None else int(value)))


def get_option(name: str) -> int:
    v = C.c_int64()
    _check(lib().tsdbhip_get_option(name.encode(), C.byref(v)))
    return v.value


def debug_buffers() -> abi.BufferCounts:
    """tsdbhip_debug_buffers: live device buffers and their bytes, live page-locked buffers and
    theirs, over every context of the process (tests: a closed engine leaves none behind)."""
    dn, db, hn, hb = C.c_int64(), C.c_uint64(), C.c_int64(), C.c_uint64()
    _check(lib().tsdbhip_debug_buffers(C.byref(dn), C.byref(db), C.byref(hn), C.byref(hb)))
    return abi.BufferCounts(dn.value, db.value, hn.value, hb.value)


def reset_options() -> None:
    for n in OPTIONS:
        set_option(n, -1)


class options:
    """Context manager: developer options set for the block, their previous values restored
    after it (so blocks nest)."""

    def __init__(self, **kw):
        self.kw = kw
        self.old = {}

    def __enter__(self):
        self.old = {k: get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            set_option(k, v)
        return False


def parse_downsample(spec: str) -> abi.Query:
    q = abi.new_query(0, 0)
    _check(lib().tsdbhip_parse_downsample(spec.encode(), C.byref(q)))
    return q


def scan_bounds(q: abi.Query):
    s, e = C.c_int64(), C.c_int64()
    _check(lib().tsdbhip_scan_bounds(C.byref(q), C.byref(s), C.byref(e)))
    return s.value, e.value


def shard_bounds(batch: abi.HostBatch, world: int, mode: int = SHARD_SERIES):
    """tsdbhip_shard_bounds: world + 1 byte-balanced boundaries (host logic, no GPU needed)."""
    b = np.zeros(world + 1, np.int64)
    _check(lib().tsdbhip_shard_bounds(C.byref(batch.c), world, mode, b.ctypes.data))
    return b


def rollup_interval(interval: str, row_span: str) -> abi.RollupInterval:
    """RollupInterval.builder().setInterval(interval).setRowSpan(row_span).build()."""
    iv = abi.RollupInterval()
    _check(lib().tsdbhip_rollup_interval_parse(interval.encode(), row_span.encode(), C.byref(iv)))
    return iv


def rollup_basetime(timestamp: int, iv: abi.RollupInterval) -> int:
    """RollupUtils.getRollupBasetime."""
    out = C.c_int32()
    _check(lib().tsdbhip_rollup_basetime(timestamp, C.byref(iv), C.byref(out)))
    return out.value


def rollup_qualifier(timestamp: int, basetime: int, flags: int, aggregator_id: int, iv: abi.RollupInterval) -> bytes:
    """RollupUtils.buildRollupQualifier."""
    out = (C.c_uint8 * 3)()
    _check(lib().tsdbhip_rollup_qualifier(timestamp, basetime, flags, aggregator_id, C.byref(iv), out))
    return bytes(out)


class RollupCells:
    """Cells of one rollup generation, in (function, series, time) order."""

    def __init__(self, series, base_time, qualifier, val_off, value):
        self.series = series          # int32 [n] batch series index
        self.base_time = base_time    # uint32 [n] row base time (s)
        self.qualifier = qualifier    # uint8 [n, 3]
        self.val_off = val_off        # uint64 [n + 1]
        self.value = value            # uint8 [val_off[-1]]

    def __len__(self):
        return len(self.series)

    def cell(self, i):
        """(series, base_time, qualifier bytes, value bytes) of cell i."""
        return (int(self.series[i]), int(self.base_time[i]), bytes(self.qualifier[i]),
                bytes(self.value[self.val_off[i]:self.val_off[i + 1]]))


class PreaggCells:
    """Cells of one pre-aggregate generation, in (function, group, time) order."""

    def __init__(self, func_index, group, base_time, qual_off, qualifier, val_off, value):
        self.func_index = func_index  # int32 [n] index into the spec's functions
        self.group = group            # int32 [n] batch group id
        self.base_time = base_time    # uint32 [n] row base time (s)
        self.qual_off = qual_off      # uint64 [n + 1]
        self.qualifier = qualifier    # uint8 [qual_off[-1]]: 3 bytes a cell (rollup interval) or 2
        self.val_off = val_off        # uint64 [n + 1]
        self.value = value            # uint8 [val_off[-1]]

    def __len__(self):
        return len(self.group)

    def cell(self, i):
        """(func_index, group, base_time, qualifier bytes, value bytes) of cell i."""
        return (int(self.func_index[i]), int(self.group[i]), int(self.base_time[i]),
                bytes(self.qualifier[self.qual_off[i]:self.qual_off[i + 1]]),
                bytes(self.value[self.val_off[i]:self.val_off[i + 1]]))


class _ResultOwner:
    """Frees a tsdbhip_result when the numpy views into it are gone."""

    def __init__(self, res):
        self.res = res
        self.free = lib().tsdbhip_result_free

    def __del__(self):
        if self.res:
            self.free(self.res)
            self.res = None


class Engine:
    """One tsdbhip context bound to one GPU -- or, with `devices`, one multi-device context
    (tsdbhip_init_devices) that shards every load over those GPUs and answers queries as one GPU
    would."""

    def __init__(self, device: int = 0, devices=None, transport: int = MD_AUTO):
        self.ctx = C.c_void_p()
        if devices is None:
            _check(lib().tsdbhip_init(device, C.byref(self.ctx)))
        else:
            arr = np.ascontiguousarray(devices, dtype=np.int32)
            _check(lib().tsdbhip_init_devices(arr.ctypes.data, len(arr), transport, C.byref(self.ctx)))
            device = int(arr[0])
        self.device = device
        self.devices = None if devices is None else [int(d) for d in devices]
        self._batch = None
        self.last_call_ms = 0.0

    def shard_mode(self, mode: int):
        """tsdbhip_md_shard_mode: SHARD_AUTO / SHARD_SERIES / SHARD_GROUPS for the next loads."""
        _check(lib().tsdbhip_md_shard_mode(self.ctx, mode))

    def md_info(self):
        """tsdbhip_md_info -> (n_devices, transport, shard mode of the resident batch, series per device)."""
        nd, tr, mode = C.c_int(), C.c_int(), C.c_int()
        _check(lib().tsdbhip_md_info(self.ctx, C.byref(nd), C.byref(tr), C.byref(mode), None))
        per = np.zeros(nd.value, np.int64)
        _check(lib().tsdbhip_md_info(self.ctx, None, None, None, per.ctypes.data))
        return nd.value, tr.value, mode.value, per

    def md_stats(self):
        """tsdbhip_md_stats -> (per-device Timing list, RCCL communicator ranks, device-to-device
        bytes) of the last run on a multi-device context."""
        nd = C.c_int()   # (n_devices only: md_info's per-device series walks the shards)
        _check(lib().tsdbhip_md_info(self.ctx, C.byref(nd), None, None, None))
        nd = nd.value
        per = (abi.Timing * nd)()
        ranks, xb = C.c_int(), C.c_double()
        _check(lib().tsdbhip_md_stats(self.ctx, C.cast(per, C.c_void_p), C.byref(ranks), C.byref(xb)))
        return list(per), ranks.value, xb.value

    def close(self):
        if self.ctx:
            lib().tsdbhip_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load(self, batch: abi.HostBatch):
        _check(lib().tsdbhip_load(self.ctx, C.byref(batch.c)))
        self._batch = batch

    def regroup(self, group_ids):
        """tsdbhip_regroup: new group ids for the loaded series, in the order of the batch given to
        the load (abi.GROUP_NONE: no group-by tag, abi.GROUP_EXCLUDED: filtered out).  The cells
        stay where they are; the next queries see the restricted, regrouped batch."""
        ids = np.ascontiguousarray(group_ids, dtype=np.int32)
        if ids.ndim != 1:
            raise ValueError("group_ids must be one-dimensional")
        _check(lib().tsdbhip_regroup(self.ctx, ids.ctypes.data, len(ids)))

    def append(self, delta: abi.HostBatch, series_index, series_new) -> abi.AppendInfo:
        """tsdbhip_append: the delta's rows appended to the resident batch (a row with the base
        time of its series' last resident row replaces it).  series_index[i] is delta series i's
        index in the batch after the append, series_new[i] marks a series not resident so far;
        from then on Engine.regroup's ids are in the new index space."""
        idx = np.ascontiguousarray(series_index, dtype=np.int64)
        new = np.ascontiguousarray(np.asarray(series_new) != 0, dtype=np.uint8)
        if idx.ndim != 1 or idx.shape != new.shape or len(idx) != delta.n_series:
            raise ValueError("series_index and series_new need one entry a delta series")
        info = abi.AppendInfo()
        # (an empty array's data pointer may be null: the library wants non-null pointers only with series)
        _check(lib().tsdbhip_append(self.ctx, C.byref(delta.c), idx.ctypes.data if len(idx) else None,
                                    new.ctypes.data if len(new) else None, C.byref(info)))
        return info

    def upsert(self, delta: abi.HostBatch, series_index, series_new) -> abi.UpsertInfo:
        """tsdbhip_upsert: the delta's rows upserted by (series, base time) anywhere in the resident
        batch -- a row with the base time of any resident row of its series replaces it, every
        other row is inserted where base order puts it.  series_index and series_new as for
        append."""
        idx = np.ascontiguousarray(series_index, dtype=np.int64)
        new = np.ascontiguousarray(np.asarray(series_new) != 0, dtype=np.uint8)
        if idx.ndim != 1 or idx.shape != new.shape or len(idx) != delta.n_series:
            raise ValueError("series_index and series_new need one entry a delta series")
        info = abi.UpsertInfo()
        _check(lib().tsdbhip_upsert(self.ctx, C.byref(delta.c), idx.ctypes.data if len(idx) else None,
                                    new.ctypes.data if len(new) else None, C.byref(info)))
        return info

    def put(self, points, fix_duplicates: bool = False) -> abi.PutInfo:
        """tsdbhip_put: datapoint writes merged into the resident rows on the device, as a scan of
        the store after the same TSDB.addPoint calls would compact them.  points: in write order, an
        abi.POINT_DTYPE array or [(series_index, timestamp, kind, value), ...] (abi.make_points);
        series_index is a batch index in the present numbering, of a resident series."""
        if not (isinstance(points, np.ndarray) and points.dtype == abi.POINT_DTYPE):
            points = abi.make_points(points)
        pts = np.ascontiguousarray(points)
        if pts.ndim != 1:
            raise ValueError("points must be one-dimensional")
        info = abi.PutInfo()
        _check(lib().tsdbhip_put(self.ctx, pts.ctypes.data if len(pts) else None, len(pts),
                                 abi.PUT_FIX_DUPLICATES if fix_duplicates else 0, C.byref(info)))
        return info

    def trim(self, cutoff_s: int, pack_dead_pct: int = abi.TRIM_NO_PACK) -> abi.TrimInfo:
        """tsdbhip_trim: every resident row with a base time below cutoff_s is evicted (series and
        ids stay, a series may be left without rows).  pack_dead_pct < 0 never moves a cell byte;
        otherwise the blobs are re-laid without their dead bytes when those are at least that per
        cent of the used bytes (0: always)."""
        info = abi.TrimInfo()
        _check(lib().tsdbhip_trim(self.ctx, int(cutoff_s), int(pack_dead_pct), C.byref(info)))
        return info

    def remove(self, ranges, drop_empty: bool = False, pack_dead_pct: int = abi.TRIM_NO_PACK):
        """tsdbhip_remove: the rows of `ranges` -- (series_index, from_s, to_s) triples, the index in
        the batch numbering before the call -- leave the resident batch wherever they sit; with
        drop_empty every series left without a row is retired and the batch renumbered.
        pack_dead_pct as for trim.  Returns (abi.RemoveInfo, new_index): new_index[i] is series
        i's batch index after the call, -1 for a retired one."""
        ranges = list(ranges)
        arr = (abi.RemoveRange * max(1, len(ranges)))()
        for k, (i, a, b) in enumerate(ranges):
            arr[k] = abi.RemoveRange(int(i), int(a), int(b))
        n = C.c_int64(0)
        # every loaded series, excluded ones included (a context the hook refuses is refused by the call itself)
        if lib().tsdbhip_debug_loaded(self.ctx, C.byref(n), None) != 0:
            n = C.c_int64(0)
        new_index = np.full(n.value, -1, dtype=np.int64)
        info = abi.RemoveInfo()
        _check(lib().tsdbhip_remove(self.ctx, C.cast(arr, C.c_void_p) if ranges else None, len(ranges),
                                    abi.REMOVE_DROP_EMPTY if drop_empty else 0, int(pack_dead_pct),
                                    new_index.ctypes.data if len(new_index) else None, C.byref(info)))
        return info, new_index

    def last(self, series_index=None, anchor_s: int = 0, anchor_each=None, back_scan: int = 0):
        """tsdbhip_last: the newest datapoint of each selected series at or before its anchor hour,
        looking back over at most back_scan hour rows (/api/query/last).  series_index: batch indices
        in the present numbering, any order, repeats allowed; None: every loaded series in batch
        order.  anchor_each: one anchor (s) a selected series instead of anchor_s.  Returns
        (ts_ms int64, bits uint64, kind uint8, abi.LastInfo): kind abi.LAST_INT -> bits is the long,
        abi.LAST_FLOAT -> the double's bits, abi.LAST_NONE -> no answer (ts_ms = bits = 0)."""
        if series_index is None:
            n = C.c_int64(0)
            # every loaded series, excluded ones included (a context the hook refuses is refused by the call itself)
            if lib().tsdbhip_debug_loaded(self.ctx, C.byref(n), None) != 0:
                n = C.c_int64(0)
            sel, n_sel = None, n.value
        else:
            sel = np.ascontiguousarray(series_index, dtype=np.int64)
            if sel.ndim != 1:
                raise ValueError("series_index must be one-dimensional")
            n_sel = len(sel)
        each = None
        if anchor_each is not None:
            each = np.ascontiguousarray(anchor_each, dtype=np.int64)
            if each.shape != (n_sel,):
                raise ValueError("anchor_each needs one entry a selected series")
        # (an empty array's data pointer may be null: the outputs are allocated with one entry at least)
        ts = np.zeros(max(1, n_sel), np.int64)
        bits = np.zeros(max(1, n_sel), np.uint64)
        kind = np.zeros(max(1, n_sel), np.uint8)
        info = abi.LastInfo()
        t0 = time.perf_counter()
        # (a null selection means every series: an empty one is handed over as some non-null pointer)
        sel_p = None if sel is None else sel.ctypes.data if n_sel else ts.ctypes.data
        _check(lib().tsdbhip_last(self.ctx, sel_p, n_sel, int(anchor_s), each.ctypes.data if each is not None and n_sel else None,
                                  int(back_scan), ts.ctypes.data, bits.ctypes.data, kind.ctypes.data, C.byref(info)))
        self.last_call_ms = (time.perf_counter() - t0) * 1e3
        return ts[:n_sel], bits[:n_sel], kind[:n_sel], info

    def load_tags(self, tag_ptr, tagk, tagv):
        """tsdbhip_tags_load: the loaded series' tags in batch order -- tag_ptr[n + 1] from 0, the
        tagk / tagv UIDs as unsigned integers, tagk strictly ascending inside a series.  The table
        stays resident until a load or an edit that changes the series numbering drops it."""
        ptr = np.ascontiguousarray(tag_ptr, dtype=np.int64)
        k = np.ascontiguousarray(tagk, dtype=np.uint32)
        v = np.ascontiguousarray(tagv, dtype=np.uint32)
        if ptr.ndim != 1 or len(ptr) < 1 or k.ndim != 1 or k.shape != v.shape:
            raise ValueError("tag_ptr needs n + 1 entries, tagk and tagv one entry a tag")
        if len(k) < int(ptr[-1]):
            raise ValueError("tag_ptr points past the end of tagk / tagv")
        t = abi.TagTable(len(ptr) - 1, ptr.ctypes.data, k.ctypes.data if len(k) else None, v.ctypes.data if len(v) else None)
        _check(lib().tsdbhip_tags_load(self.ctx, C.byref(t)))

    def tags_loaded(self):
        """tsdbhip_tags_loaded: (series, tags) of the resident tag table, (0, 0) without one."""
        n, t = C.c_int64(0), C.c_int64(0)
        _check(lib().tsdbhip_tags_loaded(self.ctx, C.byref(n), C.byref(t)))
        return n.value, t.value

    def regroup_tags(self, filters, group_by=(), explicit_tags: bool = False, dry: bool = False):
        """tsdbhip_regroup_tags: the tag filters evaluated, the group keys extracted and numbered in
        ByteMap order and the batch regrouped, all on the device.  filters: an abi.HostTagQuery, or
        [(tagk uid, abi.TF_*, ascending tagv uids), ...] with group_by (ascending tagk uids) and
        explicit_tags.  dry: compute and report only.  Returns (ids int32 in batch order, keys -- the
        distinct group keys as tuples of tagv uids, in id order --, abi.TagsInfo)."""
        q = filters if isinstance(filters, abi.HostTagQuery) else abi.HostTagQuery(filters, group_by, explicit_tags)
        n = C.c_int64(0)
        # every loaded series, excluded ones included (a context the hook refuses is refused by the call itself)
        if lib().tsdbhip_debug_loaded(self.ctx, C.byref(n), None) != 0:
            n = C.c_int64(0)
        ids = np.zeros(max(1, n.value), np.int32)
        info = abi.TagsInfo()
        _check(lib().tsdbhip_regroup_tags(self.ctx, C.byref(q.c), abi.TAGS_DRY if dry else 0, ids.ctypes.data, C.byref(info)))
        ngb = len(q.group_by_list)
        kw = np.zeros(max(1, info.n_groups * ngb), np.uint32)
        _check(lib().tsdbhip_tags_keys(self.ctx, kw.ctypes.data))
        keys = [tuple(int(x) for x in kw[g * ngb:(g + 1) * ngb]) for g in range(info.n_groups)]
        return ids[:n.value], keys, info

    def load_cells(self, cb: abi.HostCellBatch):
        """tsdbhip_load_cells: the scan's rows compacted on the GPU become the resident batch."""
        _check(lib().tsdbhip_load_cells(self.ctx, C.byref(cb.c)))
        self._batch = cb

    def load_histograms(self, hb: "H.HostHistBatch"):
        """tsdbhip_load_histograms: the resident histogram store."""
        _check(lib().tsdbhip_load_histograms(self.ctx, C.byref(hb.c)))

    def run_histogram(self, q: abi.Query, percentiles=(), show_buckets: bool = False, span_range=None):
        """TsdbQuery.runHistogram over the resident histogram store: per emitted group the list
        of its DataPoints (percentile series, then bucket series), see histogram.result_to_series.
        span_range=(start_ms, end_ms): HistogramAggregationIterator bounds given directly
        (tsdbhip_hist_run_range, every row)."""
        pct = (C.c_float * max(1, len(percentiles)))(*[float(x) for x in percentiles])
        res = C.POINTER(H.HistResult)()
        if span_range is None:
            _check(lib().tsdbhip_hist_run(self.ctx, C.byref(q), len(percentiles), pct, int(bool(show_buckets)),
                                          C.byref(res)))
        else:
            _check(lib().tsdbhip_hist_run_range(self.ctx, C.byref(q), int(span_range[0]), int(span_range[1]),
                                                len(percentiles), pct, int(bool(show_buckets)), C.byref(res)))
        try:
            return H.result_to_series(res.contents, [float(C.c_float(x).value) for x in percentiles])
        finally:
            lib().tsdbhip_hist_result_free(res)

    def load_rollup(self, rb: abi.HostRollupBatch):
        """tsdbhip_load_rollup: a rollup table's scan result as the resident batch; run()
        then answers rollup queries over it."""
        _check(lib().tsdbhip_load_rollup(self.ctx, C.byref(rb.c)))
        self._batch = rb

    def synth(self, n_series: int, start_s: int, n_points: int, period_ms: int, value_kind: int = 0,
              n_groups: int = 1, int_mod: int = 2000, seed: int = 0x5EED):
        sp = abi.SynthSpec(n_series, start_s, n_points, period_ms, value_kind, n_groups, int_mod, seed)
        _check(lib().tsdbhip_synth(self.ctx, C.byref(sp)))

    def synth_shard(self, pos_begin: int, pos_end: int, n_series: int, start_s: int, n_points: int,
                    period_ms: int, value_kind: int = 0, n_groups: int = 1, int_mod: int = 2000, seed: int = 0x5EED):
        """Batch positions [pos_begin, pos_end) of the n_series synthetic store (one rank's shard)."""
        sp = abi.SynthSpec(n_series, start_s, n_points, period_ms, value_kind, n_groups, int_mod, seed)
        _check(lib().tsdbhip_synth_shard(self.ctx, C.byref(sp), pos_begin, pos_end))

    def load_shard(self, batch: abi.HostBatch, mode: int, begin: int, end: int):
        """tsdbhip_load_shard: range [begin, end) of the batch under a TSDB_SHARD_* mode."""
        _check(lib().tsdbhip_load_shard(self.ctx, C.byref(batch.c), mode, begin, end))
        self._batch = batch

    def download(self) -> abi.HostBatch:
        ns, nr, qb, vb = C.c_int64(), C.c_int64(), C.c_uint64(), C.c_uint64()
        _check(lib().tsdbhip_batch_sizes(self.ctx, C.byref(ns), C.byref(nr), C.byref(qb), C.byref(vb)))
        srp = np.zeros(ns.value + 1, np.int64)
        base = np.zeros(max(1, nr.value), np.uint32)
        qo = np.zeros(nr.value + 1, np.uint64)
        vo = np.zeros(nr.value + 1, np.uint64)
        q = np.zeros(max(1, qb.value), np.uint8)
        v = np.zeros(max(1, vb.value), np.uint8)
        g = np.zeros(max(1, ns.value), np.int32)
        _check(lib().tsdbhip_batch_download(self.ctx, srp.ctypes.data, base.ctypes.data, qo.ctypes.data,
                                            vo.ctypes.data, q.ctypes.data, v.ctypes.data, g.ctypes.data))
        return abi.HostBatch(srp, base[:nr.value], qo, vo, q[:qb.value], v[:vb.value], g[:ns.value])

    def n_series(self) -> int:
        ns, nr, qb, vb = C.c_int64(), C.c_int64(), C.c_uint64(), C.c_uint64()
        _check(lib().tsdbhip_batch_sizes(self.ctx, C.byref(ns), C.byref(nr), C.byref(qb), C.byref(vb)))
        return ns.value

    def resident_groups(self) -> np.ndarray:
        """Group id of every resident series position (the resident order is group-sorted)."""
        n = self.n_series()
        g = np.zeros(max(1, n), np.int32)
        _check(lib().tsdbhip_batch_download_range(self.ctx, 0, n, None, None, None, None, None, None,
                                                  g.ctypes.data))
        return g[:n]

    def download_range(self, s0: int, s1: int) -> abi.HostBatch:
        """Resident series positions [s0, s1) as a host batch (group ids kept)."""
        nr, qb, vb = C.c_int64(), C.c_uint64(), C.c_uint64()
        _check(lib().tsdbhip_batch_range_sizes(self.ctx, s0, s1, C.byref(nr), C.byref(qb), C.byref(vb)))
        srp = np.zeros(s1 - s0 + 1, np.int64)
        base = np.zeros(max(1, nr.value), np.uint32)
        qo = np.zeros(nr.value + 1, np.uint64)
        vo = np.zeros(nr.value + 1, np.uint64)
        q = np.zeros(max(1, qb.value), np.uint8)
        v = np.zeros(max(1, vb.value), np.uint8)
        g = np.zeros(max(1, s1 - s0), np.int32)
        _check(lib().tsdbhip_batch_download_range(self.ctx, s0, s1, srp.ctypes.data, base.ctypes.data,
                                                  qo.ctypes.data, vo.ctypes.data, q.ctypes.data, v.ctypes.data,
                                                  g.ctypes.data))
        return abi.HostBatch(srp, base[:nr.value], qo, vo, q[:qb.value], v[:vb.value], g[:s1 - s0])

    def run(self, q: abi.Query):
        """tsdbhip_run -> [(group_id, ts, bits, is_int)]; the arrays are views into the
        library's result, freed when the last of them is garbage-collected."""
        res = C.POINTER(abi.Result)()
        t = time.perf_counter()
        _check(lib().tsdbhip_run(self.ctx, C.byref(q), C.byref(res)))
        self.last_call_ms = (time.perf_counter() - t) * 1000.0   # the C call alone (host wall time)
        return abi.result_to_groups(res.contents, owner=_ResultOwner(res))

    def run_multi(self, queries):
        """tsdbhip_run_multi: one decode + downsample pass shared by several queries."""
        n = len(queries)
        arr = (abi.Query * n)(*queries)
        outs = (C.POINTER(abi.Result) * n)()
        t = time.perf_counter()
        _check(lib().tsdbhip_run_multi(self.ctx, arr, n, outs))
        self.last_call_ms = (time.perf_counter() - t) * 1000.0   # the C call alone (host wall time)
        return [abi.result_to_groups(outs[i].contents, owner=_ResultOwner(outs[i])) for i in range(n)]

    def run_rollup_batch(self, rb: abi.HostRollupBatch, q: abi.Query):
        self.load_rollup(rb)
        return self.run(q)

    def run_batch(self, batch: abi.HostBatch, q: abi.Query):
        """Runner for TsdbQuery: load the query's spans, then run."""
        self.load(batch)
        return self.run(q)

    def timing(self) -> abi.Timing:
        t = abi.Timing()
        _check(lib().tsdbhip_last_timing(self.ctx, C.byref(t)))
        return t

    def sync(self):
        _check(lib().tsdbhip_sync(self.ctx))

    def debug_rows(self):
        """Test hook: k_index's per-row (ndp, flags, lsb, absmax) of the resident batch."""
        ns, nr, qb, vb = C.c_int64(), C.c_int64(), C.c_uint64(), C.c_uint64()
        _check(lib().tsdbhip_batch_sizes(self.ctx, C.byref(ns), C.byref(nr), C.byref(qb), C.byref(vb)))
        n = max(1, nr.value)
        ndp, flags = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        lsb, amax = np.zeros(n, np.int32), np.zeros(n, np.float64)
        _check(lib().tsdbhip_debug_rows(self.ctx, ndp.ctypes.data, flags.ctypes.data, lsb.ctypes.data,
                                        amax.ctypes.data))
        k = nr.value
        return ndp[:k], flags[:k], lsb[:k], amax[:k]

    def debug_regular(self):
        """Test hook: (first_step [rows, 2] uint32 -- a regular row's first offset and step in
        seconds, step 0 = not regular --, tiles on each class's regular list [2], tiles the last
        query launched through k_fast's values-only form)."""
        ns, nr, qb, vb = C.c_int64(), C.c_int64(), C.c_uint64(), C.c_uint64()
        _check(lib().tsdbhip_batch_sizes(self.ctx, C.byref(ns), C.byref(nr), C.byref(qb), C.byref(vb)))
        fs = np.zeros((max(1, nr.value), 2), np.uint32)
        lists, launched = np.zeros(2, np.int64), C.c_int64()
        _check(lib().tsdbhip_debug_regular(self.ctx, fs.ctypes.data, lists.ctypes.data, C.byref(launched)))
        return fs[:nr.value], lists, launched.value

    def debug_layout(self):
        """Test hook: (qoff, voff) of every loaded row in the device blobs, rows in descriptor
        order -- the visible series' rows in resident order, then the excluded series'."""
        nr = C.c_int64()
        _check(lib().tsdbhip_debug_loaded(self.ctx, None, C.byref(nr)))
        qoff, voff = np.zeros(max(1, nr.value), np.uint64), np.zeros(max(1, nr.value), np.uint64)
        _check(lib().tsdbhip_debug_layout(self.ctx, qoff.ctypes.data, voff.ctypes.data))
        return qoff[:nr.value], voff[:nr.value]

    def debug_index(self):
        """Test hook: (cnt, fused) of the last load's index -- cnt[0..10] rows by index class,
        cnt[IDX_C_SHORT4] / cnt[IDX_C_SHORTV] k_index_short's rows, cnt[IDX_C_FAIL] the rows it
        handed back; fused: the classifying pass indexed the short rows itself."""
        cnt, fused = np.zeros(16, np.uint32), C.c_int()
        _check(lib().tsdbhip_debug_index(self.ctx, cnt.ctypes.data, C.byref(fused)))
        return cnt, fused.value

    def debug_sel_window(self):
        """Test hook: (runs, misses) of the sampled-window percentile group-by select."""
        runs, misses = C.c_int64(), C.c_int64()
        _check(lib().tsdbhip_debug_sel_window(self.ctx, C.byref(runs), C.byref(misses)))
        return runs.value, misses.value

    def debug_rollup(self):
        """Test hook: the last rollup_run's route -- (streaming pass launched 0 / 1, series it was
        launched over, series its first row class handed back, series k_rollup_agg reduced)."""
        out = np.zeros(4, np.int64)
        _check(lib().tsdbhip_debug_rollup(self.ctx, out.ctypes.data))
        return tuple(int(x) for x in out)

    def debug_pct(self):
        """Test hook: the last percentile-downsampling run's route -- (k_pct_rows launched 0 / 1,
        its KEYS variant or -1, series it handed back, series sent to the large-bucket pass, that
        pass's waves, its big_cap)."""
        out = np.zeros(6, np.int64)
        _check(lib().tsdbhip_debug_pct(self.ctx, out.ctypes.data))
        return tuple(int(x) for x in out)

    # ---- rollup generation (tsdbhip_rollup_run) ----
    def rollup_run(self, interval: abi.RollupInterval, start_s: int, end_s: int,
                   funcs=(("sum", 0), ("count", 1), ("max", 2), ("min", 3))):
        """Generates the rollup cells of the resident batch on the device; returns
        (n_cells, value_bytes).  funcs = [(downsample function, rollup aggregator id)]."""
        sp = abi.RollupSpec()
        sp.interval = interval
        sp.start_s = start_s
        sp.end_s = end_s
        sp.n_funcs = len(funcs)
        for i, (fn, aid) in enumerate(funcs):
            sp.func[i] = abi.AGG[fn] if isinstance(fn, str) else fn
            sp.agg_id[i] = aid
        n, b = C.c_int64(), C.c_uint64()
        _check(lib().tsdbhip_rollup_run(self.ctx, C.byref(sp), C.byref(n), C.byref(b)))
        return n.value, b.value

    def rollup_download(self, n_cells: int, value_bytes: int) -> RollupCells:
        series = np.zeros(max(1, n_cells), np.int32)
        base = np.zeros(max(1, n_cells), np.uint32)
        qual = np.zeros((max(1, n_cells), 3), np.uint8)
        voff = np.zeros(n_cells + 1, np.uint64)
        val = np.zeros(max(1, value_bytes), np.uint8)
        _check(lib().tsdbhip_rollup_download(self.ctx, series.ctypes.data, base.ctypes.data, qual.ctypes.data,
                                             voff.ctypes.data, val.ctypes.data))
        return RollupCells(series[:n_cells], base[:n_cells], qual[:n_cells], voff, val[:value_bytes])

    def rollup(self, interval: abi.RollupInterval, start_s: int, end_s: int,
               funcs=(("sum", 0), ("count", 1), ("max", 2), ("min", 3))) -> RollupCells:
        return self.rollup_download(*self.rollup_run(interval, start_s, end_s, funcs))

    # ---- pre-aggregate generation (tsdbhip_preagg_run) ----
    def preagg_run(self, interval, start_s: int, end_s: int, groupby_aggregator="sum",
                   funcs=(("sum", 0), ("count", 1), ("max", 2), ("min", 3)), flags: int = 0, ds_interval_ms: int = 0):
        """Generates the pre-aggregate (group-by) cells of the resident batch on the device;
        returns (n_cells, qual_bytes, value_bytes).  interval: a RollupInterval -> the cells of
        its group-by table, funcs = [(rollup function, rollup aggregator id)]; None -> the default
        interval's group-by table at ds_interval_ms, funcs = [(downsampling function, ignored)]."""
        sp = abi.PreaggSpec()
        if interval is not None:
            sp.interval = interval
        sp.ds_interval_ms = ds_interval_ms
        sp.start_s = start_s
        sp.end_s = end_s
        sp.groupby_aggregator = (abi.AGG[groupby_aggregator] if isinstance(groupby_aggregator, str)
                                 else groupby_aggregator)
        sp.flags = flags
        sp.n_funcs = len(funcs)
        for i, (fn, aid) in enumerate(funcs[:4]):
            sp.func[i] = abi.AGG[fn] if isinstance(fn, str) else fn
            sp.agg_id[i] = aid
        n, qb, vb = C.c_int64(), C.c_uint64(), C.c_uint64()
        _check(lib().tsdbhip_preagg_run(self.ctx, C.byref(sp), C.byref(n), C.byref(qb), C.byref(vb)))
        return n.value, qb.value, vb.value

    def preagg_download(self, n_cells: int, qual_bytes: int, value_bytes: int) -> PreaggCells:
        fi = np.zeros(max(1, n_cells), np.int32)
        grp = np.zeros(max(1, n_cells), np.int32)
        base = np.zeros(max(1, n_cells), np.uint32)
        qoff = np.zeros(n_cells + 1, np.uint64)
        qual = np.zeros(max(1, qual_bytes), np.uint8)
        voff = np.zeros(n_cells + 1, np.uint64)
        val = np.zeros(max(1, value_bytes), np.uint8)
        _check(lib().tsdbhip_preagg_download(self.ctx, fi.ctypes.data, grp.ctypes.data, base.ctypes.data,
                                             qoff.ctypes.data, qual.ctypes.data, voff.ctypes.data, val.ctypes.data))
        return PreaggCells(fi[:n_cells], grp[:n_cells], base[:n_cells], qoff, qual[:qual_bytes], voff,
                           val[:value_bytes])

    def preagg(self, interval, start_s: int, end_s: int, groupby_aggregator="sum",
               funcs=(("sum", 0), ("count", 1), ("max", 2), ("min", 3)), flags: int = 0,
               ds_interval_ms: int = 0) -> PreaggCells:
        return self.preagg_download(*self.preagg_run(interval, start_s, end_s, groupby_aggregator, funcs, flags,
                                                     ds_interval_ms))

    # ---- multi-GPU exchange (see include/tsdbhip.h and opentsdb_amd/dist.py) ----
    def partials_layout(self, q: abi.Query, n_groups_global: int) -> abi.PartialsLayout:
        lay = abi.PartialsLayout()
        _check(lib().tsdbhip_partials_layout_get(self.ctx, C.byref(q), n_groups_global, C.byref(lay)))
        return lay

    def run_partials(self, q: abi.Query, n_groups_global: int, ptr: int):
        """This shard's per-(group, slot) partial states into `ptr` (device or host memory)."""
        _check(lib().tsdbhip_run_partials(self.ctx, C.byref(q), n_groups_global, C.c_void_p(ptr)))

    def run_partials_multi(self, queries, n_groups_global: int, ptr: int):
        """Partial states of several queries sharing the downsampling, from one fused pass: query
        i's buffer at ptr + i * partials_layout(queries[i]).bytes."""
        n = len(queries)
        arr = (abi.Query * n)(*queries)
        _check(lib().tsdbhip_run_partials_multi(self.ctx, arr, n, n_groups_global, C.c_void_p(ptr)))

    def finalize(self, q: abi.Query, n_groups_global: int, ptr: int, n_ranks: int):
        """Rank-ordered merge of n_ranks gathered partial buffers at `ptr` -> groups."""
        res = C.POINTER(abi.Result)()
        _check(lib().tsdbhip_finalize(self.ctx, C.byref(q), n_groups_global, C.c_void_p(ptr), n_ranks,
                                      C.byref(res)))
        try:
            return abi.result_to_groups(res.contents)
        finally:
            lib().tsdbhip_result_free(res)


    # ---- multi-GPU percentile / median group-by (values to the owning rank) ----
    def sel_layout(self, q: abi.Query, n_groups_global: int):
        """(local spans per group [n_groups_global] int64, slots K)."""
        counts = np.zeros(max(1, n_groups_global), np.int64)
        k = C.c_int64()
        _check(lib().tsdbhip_sel_layout(self.ctx, C.byref(q), n_groups_global, counts.ctypes.data, C.byref(k)))
        return counts[:n_groups_global], int(k.value)

    def sel_run_values(self, q: abi.Query, n_groups_global: int, vals: int, uni: int, act: int):
        """Local span contributions ([g][k][i] f64), emit flags [G][K] u8, group active [G] u32."""
        _check(lib().tsdbhip_sel_run_values(self.ctx, C.byref(q), n_groups_global, C.c_void_p(vals),
                                            C.c_void_p(uni), C.c_void_p(act)))

    def sel_select(self, q: abi.Query, n_groups_global: int, vals: int, counts: np.ndarray, uni: int,
                   out_val: int, out_flag: int):
        counts = np.ascontiguousarray(counts, np.int64)
        _check(lib().tsdbhip_sel_select(self.ctx, C.byref(q), n_groups_global, C.c_void_p(vals),
                                        C.c_void_p(counts.ctypes.data), C.c_void_p(uni), C.c_void_p(out_val),
                                        C.c_void_p(out_flag)))

    def assemble(self, q: abi.Query, n_groups_global: int, val: int, flag: int, act: int):
        res = C.POINTER(abi.Result)()
        _check(lib().tsdbhip_assemble(self.ctx, C.byref(q), n_groups_global, C.c_void_p(val), C.c_void_p(flag),
                                      C.c_void_p(act), C.byref(res)))
        try:
            return abi.result_to_groups(res.contents)
        finally:
            lib().tsdbhip_result_free(res)


_default = None


def default_engine() -> Engine:
    global _default
    if _default is None:
        _default = Engine(int(os.environ.get("TSDBHIP_DEVICE", "0")))
    return _default
