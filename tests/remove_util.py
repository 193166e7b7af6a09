"""Host-side expectation of tsdbhip_remove, pure numpy: remove_batch gives the batch a fresh load
would be handed after the call -- the rows of every (series, from_s, to_s) range dropped and, with
drop_empty, every series without a row retired -- and the new index of every series (-1: retired)."""
from __future__ import annotations

import numpy as np

from opentsdb_amd import abi


def remove_batch(batch, ranges, drop_empty=False):
    nr, n = batch.n_rows, batch.n_series
    base = batch.row_base_time[:nr].astype(np.int64)
    ser = np.repeat(np.arange(n, dtype=np.int64), np.diff(batch.series_row_ptr))
    # the rows by (series, base); each range is an interval of that order, counted in a difference array
    rg = np.asarray(list(ranges), np.int64).reshape(-1, 3)
    key = (ser << 33) + base
    order = np.argsort(key, kind="stable")
    skey = key[order]
    lo = np.searchsorted(skey, (rg[:, 0] << 33) + np.clip(rg[:, 1], 0, 1 << 32))
    hi = np.searchsorted(skey, (rg[:, 0] << 33) + np.clip(rg[:, 2], 0, 1 << 32))
    diff = np.zeros(nr + 1, np.int64)
    np.add.at(diff, lo, 1)
    np.add.at(diff, np.maximum(hi, lo), -1)
    keep = np.ones(nr, bool)
    keep[order] = np.cumsum(diff)[:nr] == 0
    rows_of = np.bincount(ser[keep], minlength=n)
    stays = rows_of > 0 if drop_empty else np.ones(n, bool)
    new_index = np.where(stays, np.cumsum(stays) - 1, -1).astype(np.int64)
    srp = np.zeros(int(stays.sum()) + 1, np.int64)
    srp[1:] = np.cumsum(rows_of[stays])

    def gather(off, blob):
        off = off.astype(np.int64)
        starts, lens = off[:nr][keep], np.diff(off)[keep]
        new = np.zeros(len(lens) + 1, np.int64)
        new[1:] = np.cumsum(lens)
        pos = np.repeat(starts - new[:-1], lens) + np.arange(int(new[-1]), dtype=np.int64)
        return new.astype(np.uint64), blob[pos]

    qo, qb = gather(batch.row_qual_off, batch.qual)
    vo, vb = gather(batch.row_val_off, batch.val)
    out = abi.HostBatch(srp, batch.row_base_time[:nr][keep].astype(np.uint32), qo, vo, qb, vb,
                        np.asarray(batch.group_id, np.int32)[stays].copy())
    return out, new_index
