"""Host reference for /api/query/last over an abi.HostBatch: plain Python, no GPU, no ctypes.

Written from the reference's text, not from k_last.hip:

* TSUIDQuery.getLastPoint (src/meta/TSUIDQuery.java:161-217) starts at Internal.baseTime of the
  anchor, h = t - t % 3600, and LastPointCB (:609-646) asks for the row of that hour; while the row
  is missing and fewer than back_scan iterations have run, it steps one hour back (h -= 3600) and
  asks again.  The first row that exists answers; none within back_scan steps: null.  A negative
  back_scan is an IllegalArgumentException (:163-166).
* Internal.GetLastDataPointCB (src/core/Internal.java:463-495) breaks the row down with
  extractDataPoints (:237-326), which ends in Collections.sort(cells) -- a stable sort by
  Cell.compareTo, the qualifier offsets (Internal.compareQualifiers :511-519) -- and takes the
  last cell: the largest offset in ms, of equal offsets the one later in the cell.
* The timestamp is Internal.getTimestampFromQualifier (:591-603): (base + seconds) * 1000 or
  base * 1000 + milliseconds.  The value is Cell.parseValue (:139-159): a long sign-extended from
  1 / 2 / 4 / 8 bytes, or a double (a float32 widened).

The cells are decoded as tests/index_ref.py decodes them.  The hour loop runs literally inside the
series' span: the steps it would take above the series' last row are counted without being walked,
and it stops once h lies before the first row, where no further step can find one, so that a
back_scan of INT32_MAX, or an anchor far in the future, terminates.
"""
from __future__ import annotations

import numpy as np

H = 3600
KIND_NONE, KIND_INT, KIND_FLOAT = 0, 1, 2


class IllegalData(Exception):
    """The row cannot be broken down into cells (IllegalDataException)."""


def cells_of(q: bytes, v: bytes):
    """[(offset ms, is float, value bytes)] in cell order."""
    out = []
    qi = vi = 0
    if not q:
        raise IllegalData("empty qualifier array")
    while qi < len(q):
        w = 4 if (q[qi] & 0xF0) == 0xF0 else 2
        if qi + w > len(q):
            raise IllegalData("a qualifier cut short")
        if w == 4:
            off = (int.from_bytes(q[qi:qi + 4], "big") & 0x0FFFFFC0) >> 6
        else:
            off = (int.from_bytes(q[qi:qi + 2], "big") >> 4) * 1000
        fl = q[qi + w - 1] & 0xF
        qi += w
        ln = (fl & 7) + 1
        if vi + ln > len(v):
            raise IllegalData("values past the value array")
        out.append((off, (fl & 8) != 0, v[vi:vi + ln]))
        vi += ln
    return out


def parse_value(is_float: bool, b: bytes):
    """Cell.parseValue -> (kind, the long or the double's bits as an unsigned 64-bit int)."""
    if is_float:
        if len(b) == 4:
            # the float32 widened as the hardware widens it (numpy's cast, as Java's f2d)
            return KIND_FLOAT, int(np.frombuffer(b, ">f4").astype(np.float64).view(np.uint64)[0])
        if len(b) == 8:
            return KIND_FLOAT, int.from_bytes(b, "big")
        raise IllegalData("a float of %d bytes" % len(b))
    if len(b) not in (1, 2, 4, 8):
        raise IllegalData("an integer of %d bytes" % len(b))
    return KIND_INT, int.from_bytes(b, "big", signed=True) & 0xFFFFFFFFFFFFFFFF


def last_of_row(base: int, q: bytes, v: bytes):
    """(ts_ms, kind, bits) of the row's last datapoint."""
    cells = cells_of(q, v)
    order = sorted(range(len(cells)), key=lambda i: cells[i][0])   # stable, as Collections.sort
    off, is_float, b = cells[order[-1]]
    kind, bits = parse_value(is_float, b)
    return base * 1000 + off, kind, bits


def series_rows(batch, s: int):
    """{base: (qualifiers, values)} of series s of an abi.HostBatch."""
    srp = np.asarray(batch.series_row_ptr).astype(np.int64)
    qo = np.asarray(batch.row_qual_off).astype(np.int64)
    vo = np.asarray(batch.row_val_off).astype(np.int64)
    rows = {}
    for r in range(int(srp[s]), int(srp[s + 1])):
        rows[int(batch.row_base_time[r])] = (bytes(batch.qual[qo[r]:qo[r + 1]]), bytes(batch.val[vo[r]:vo[r + 1]]))
    return rows


def answer_base(bases, anchor_s: int, back_scan: int):
    """LastPointCB's loop over a series' row bases: the base of the first row it finds, or None."""
    if back_scan < 0:
        raise ValueError("Backscan must be zero or a positive number")
    h = anchor_s - anchor_s % H
    first = min(bases) if bases else None
    iteration = 0
    if bases and h > max(bases):
        # the steps above the series' last row find nothing: they are counted, not walked
        iteration = (h - max(bases)) // H
        if iteration > back_scan:
            return None
        h = max(bases)
    while True:
        if h in bases:
            return h
        if iteration >= back_scan or first is None or h < first:
            return None
        h -= H
        iteration += 1


def last_point(rows: dict, anchor_s: int, back_scan: int):
    """getLastPoint over one series' rows {base: (q, v)}: (ts_ms, kind, bits) or None."""
    h = answer_base(rows, anchor_s, back_scan)
    return None if h is None else last_of_row(h, *rows[h])


def last_ref(batch, series_index=None, anchor_s=0, anchor_each=None, back_scan=0):
    """What Engine.last returns without its info: (ts_ms int64, bits uint64, kind uint8)."""
    n = len(batch.series_row_ptr) - 1
    sel = list(range(n)) if series_index is None else [int(i) for i in series_index]
    ts = np.zeros(len(sel), np.int64)
    bits = np.zeros(len(sel), np.uint64)
    kind = np.zeros(len(sel), np.uint8)
    cache = {}
    for k, s in enumerate(sel):
        if s not in cache:
            cache[s] = series_rows(batch, s)
        a = int(anchor_each[k]) if anchor_each is not None else int(anchor_s)
        got = last_point(cache[s], a, back_scan)
        if got is not None:
            ts[k], kind[k], bits[k] = got[0], got[1], got[2]
    return ts, bits, kind
