"""Host reference for the load-time row index: the facts of RowDesc computed from the bytes.

Plain Python over an abi.HostBatch -- no GPU, no ctypes.  Written from the reference's cell
format, not from k_index.hip:

* a compacted cell's qualifier array is a run of 2-byte (seconds) and 4-byte (milliseconds,
  first nibble 0xF) qualifiers (Internal.inMilliseconds :621, getOffsetFromQualifier :647,
  getValueLengthFromQualifier :680, getFlagsFromQualifier :777): the low 4 bits are
  the flags -- 0x8 floating point, low 3 bits the value length - 1 -- and the rest the offset
  from the row's base time, seconds << 4 or milliseconds << 6;
* the values lie back to back in qualifier order, big-endian, a meta byte after them when
  the cell holds more than one (RowSeq.Iterator :552-614);
* integers are 1, 2, 4 or 8 bytes, floats 4 or 8: anything else is an IllegalDataException
  (RowSeq.extractIntegerValue / extractFloatingPointValue, RowSeq.java:233-266), as is a
  qualifier or a value that runs past its array.

What is a convention of the descriptor and not of the cell format is restated from engine.h:
the flag bits, the uniform value length being a property of rows of one qualifier width (it is
the stride of such a row; 0 for a mixed row), ROW_NOCERT (row_nocert, engine.h:47-50), and the
across-row rule of ROW_UNSORTED (a row whose first datapoint is not after every datapoint of
the series' earlier well-formed rows).  ROW_SFIRST is an input bit the host sets and is not
computed here.
"""
from __future__ import annotations

import math
import struct
from typing import NamedTuple

import numpy as np

INT32_MAX = 2147483647

ROW_QW_MASK, ROW_VL_SHIFT, ROW_VL_MASK = 0x7, 8, 0xF00
ROW_ERR, ROW_ALLF, ROW_NAN, ROW_NEGZ, ROW_UNSORTED, ROW_SFIRST, ROW_ALLI, ROW_VLE2, ROW_NOCERT = (
    0x10000, 0x20000, 0x40000, 0x80000, 0x100000, 0x200000, 0x400000, 0x800000, 0x1000000)
# what is compared on a malformed row (its value statistics are never read)
SHAPE_FLAGS = ROW_QW_MASK | ROW_VL_MASK | ROW_ALLF | ROW_ALLI | ROW_VLE2 | ROW_UNSORTED


class RowFacts(NamedTuple):
    ndp: int
    qw: int            # 2, 4, or 0: mixed widths (or bytes left over)
    vl: int            # the uniform value length of a row of one width, else 0
    allf: bool
    alli: bool
    vle2: bool
    nan: bool
    negz: bool
    unsorted: bool     # within the cell
    err: bool
    lsb: int
    absmax: float
    first_ms: int      # offset of the first datapoint from the base time (-1: none)
    max_ms: int        # the latest offset

    @property
    def nocert(self) -> bool:
        return row_nocert(self.lsb, self.absmax)

    def flags(self, across_unsorted: bool = False) -> int:
        f = self.qw | (self.vl << ROW_VL_SHIFT)
        for on, bit in ((self.err, ROW_ERR), (self.allf, ROW_ALLF), (self.alli, ROW_ALLI), (self.vle2, ROW_VLE2),
                        (self.nan, ROW_NAN), (self.negz, ROW_NEGZ), (self.unsorted or across_unsorted, ROW_UNSORTED),
                        (self.nocert, ROW_NOCERT)):
            if on:
                f |= bit
        return f


def lsb_exp(x: float) -> int:
    """The largest e with x / 2^e an odd integer (x finite, non-zero)."""
    m, e = math.frexp(abs(x))
    mi = int(math.ldexp(m, 53))          # exact: 2^52 <= mi < 2^53
    return e - 53 + ((mi & -mi).bit_length() - 1)


def row_nocert(lsb: int, absmax: float) -> bool:
    """engine.h row_nocert: the certificate n * absmax <= 2^(52 + lsb), n * absmax finite, fails
    already for n = 2.  For 52 + lsb > 1023 the threshold is beyond every double (math.ldexp
    raises there): only the overflow of 2 * absmax can fail the certificate."""
    if lsb == INT32_MAX or absmax == 0.0:
        return False
    na = 2.0 * absmax * (1.0 + 1e-12)
    if not na < math.inf:
        return True
    return 52 + lsb <= 1023 and na > math.ldexp(1.0, 52 + lsb)


def row_facts(q: bytes, v: bytes) -> RowFacts:
    qlen, vlen = len(q), len(v)
    err = qlen == 0
    ndp = n2 = n4 = 0
    lens = set()
    allf = alli = vle2 = True
    nan = negz = unsorted = False
    lsb, absmax = INT32_MAX, 0.0
    prev, first, mx = -1, -1, -1
    qi = vi = 0
    while qi < qlen:
        w = 4 if (q[qi] & 0xF0) == 0xF0 else 2
        if qi + w > qlen:                 # a qualifier cut short
            err = True
            break
        if w == 4:
            n4 += 1
            off = (int.from_bytes(q[qi:qi + 4], "big") & 0x0FFFFFC0) >> 6
        else:
            n2 += 1
            off = (int.from_bytes(q[qi:qi + 2], "big") >> 4) * 1000
        fl = q[qi + w - 1] & 0xF
        qi += w
        ndp += 1
        isf, ln = (fl & 8) != 0, (fl & 7) + 1
        lens.add(ln)
        allf &= isf
        alli &= not isf
        vle2 &= ln <= 2
        if off <= prev:
            unsorted = True
        prev = off
        if first < 0:
            first = off
        mx = max(mx, off)
        at, vi = vi, vi + ln
        if ln not in ((4, 8) if isf else (1, 2, 4, 8)) or vi > vlen:
            err = True
            continue
        if isf:
            x = struct.unpack(">f" if ln == 4 else ">d", v[at:vi])[0]
            if x != x:
                nan = True
                continue
            if x == 0.0 and math.copysign(1.0, x) < 0:
                negz = True
        else:
            x = float(int.from_bytes(v[at:vi], "big", signed=True))   # (a long beyond 2^53 rounds, as (double) does)
        absmax = max(absmax, abs(x))
        if x != 0.0 and not math.isinf(x):
            lsb = min(lsb, lsb_exp(x))
    qw = 2 if (ndp and n2 == ndp and qi == qlen) else 4 if (ndp and n4 == ndp and qi == qlen) else 0
    vl = next(iter(lens)) if (qw and len(lens) == 1) else 0
    return RowFacts(ndp, qw, vl, allf, alli, vle2, nan, negz, unsorted, err, lsb, absmax, first, mx)


def index_ref(batch):
    """(ndp, flags, lsb, absmax, facts) of every row of an abi.HostBatch: the arrays of
    Engine.debug_rows (flags without ROW_SFIRST), and the per-row RowFacts."""
    qual, val = bytes(np.asarray(batch.qual, np.uint8)), bytes(np.asarray(batch.val, np.uint8))
    qo = np.asarray(batch.row_qual_off).astype(np.int64)
    vo = np.asarray(batch.row_val_off).astype(np.int64)
    srp = np.asarray(batch.series_row_ptr).astype(np.int64)
    base = np.asarray(batch.row_base_time).astype(np.int64)
    nr = len(base)
    facts = [row_facts(qual[qo[r]:qo[r + 1]], val[vo[r]:vo[r + 1]]) for r in range(nr)]
    ndp, flags = np.zeros(nr, np.uint32), np.zeros(nr, np.uint32)
    lsb, absmax = np.zeros(nr, np.int32), np.zeros(nr, np.float64)
    for s in range(len(srp) - 1):
        latest = None                     # the latest datapoint of the series' earlier rows
        for r in range(int(srp[s]), int(srp[s + 1])):
            f = facts[r]
            across = False
            if not f.err and f.ndp:
                b = int(base[r]) * 1000
                across = latest is not None and b + f.first_ms <= latest
                latest = b + f.max_ms if latest is None else max(latest, b + f.max_ms)
            ndp[r], flags[r], lsb[r], absmax[r] = f.ndp, f.flags(across), f.lsb, f.absmax
    return ndp, flags, lsb, absmax, facts


# ---- cell builders shared by the index tests -------------------------------------------------
def q2(off_s: int, flags: int) -> bytes:
    """A 2-byte qualifier: seconds offset << 4 | flags."""
    return ((off_s << 4) | flags).to_bytes(2, "big")


def q4(off_ms: int, flags: int) -> bytes:
    """A 4-byte qualifier: 0xF nibble, milliseconds offset << 6 | flags."""
    return (0xF0000000 | (off_ms << 6) | flags).to_bytes(4, "big")


def one_row_batch(rows, base: int):
    """An abi.HostBatch of one-row series, one group each, from [(qualifiers, values)]."""
    from opentsdb_amd import synth
    return synth.from_series([[(base, q, v)] for q, v in rows], list(range(len(rows))))


# (name, qualifiers, values, malformed): cells a decoder must refuse, and well-formed
# neighbours of each that it must not
MALFORMED_CELLS = [
    ("odd qlen", q2(0, 0) + q2(10, 0) + b"\x00", b"\x01\x02\x00", True),
    ("truncated last qualifier in a mixed row", q2(0, 0) + q4(1500, 0)[:2], b"\x01\x02\x01", True),
    ("truncated 4-byte qualifier, 3 of 4 bytes", q4(500, 0) + q4(1500, 0)[:3], b"\x01\x02\x00", True),
    ("empty qualifier array", b"", b"", True),
    ("3-byte integer", q2(0, 2), b"\x00\x01\x02", True),
    ("3-byte integer among others", q2(0, 0) + q2(10, 2) + q2(20, 1), b"\x01\x00\x01\x02\x00\x03\x00", True),
    ("5-byte integer", q2(0, 4), b"\x00\x01\x02\x03\x04", True),
    ("2-byte float", q2(0, 0x9), b"\x3c\x00", True),
    ("values past vlen", q2(0, 1) + q2(10, 1), b"\x00\x01\x02", True),
    ("8-byte claim past vlen", q2(0, 0) + q2(10, 7) + q2(20, 0), b"\x01\x02\x03\x00", True),
    ("well-formed vle", q2(0, 0) + q2(10, 1) + q2(20, 0), b"\x01\x00\x02\x03\x00", False),
    ("well-formed mixed widths", q2(0, 0) + q4(1500, 1) + q2(3, 0xB), b"\x01\x00\x02\x3f\xc0\x00\x00\x01", False),
    ("values end exactly at vlen, no meta byte", q2(0, 1) + q2(10, 1), b"\x00\x02\x00\x04", False),
    ("spare bytes after the values", q2(0, 0) + q2(10, 0), b"\x02\x04\x00\x00\x00\x00", False),
    ("single float32", q2(7, 0xB), b"\x3f\xc0\x00\x00", False),
]
