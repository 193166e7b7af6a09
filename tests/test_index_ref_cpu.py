"""tests/index_ref.py, the host reference the GPU index tests compare RowDesc with, pinned
without a GPU by derivations that share nothing with it:

* rows written by synth.encode_rows: the facts follow from the encoder's inputs;
* hand-written byte strings with their facts as literals;
* malformed cells: the oracle (pinned to the reference's answers) raises IllegalDataException
  on a raw query over the cell exactly when the reference says ROW_ERR.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

from opentsdb_amd import abi, synth
from oracle import oracle as O
from tests import index_ref as R
from tests.index_ref import INT32_MAX, q2, q4

T0 = 1356998400


def _lsb_of_inputs(x: float) -> int:
    """Trailing zeros by repeated halving (not frexp): e with x / 2^e an odd integer."""
    e = 0
    x = abs(x)
    while x != math.floor(x):
        x *= 2.0
        e -= 1
    n = int(x)
    while n % 2 == 0:
        n //= 2
        e += 1
    return e


CASES = {
    "float32": dict(kind=1, ms=False),
    "float32 specials": dict(kind=1, ms=False, specials=True),
    "float64 ms": dict(kind=2, ms=True),
    "vle ints": dict(kind=0, ms=False, lo=-300, hi=30000),
    "1-byte ints": dict(kind=0, ms=False, lo=-128, hi=128),
    "int32 ms": dict(kind=0, ms=True, lo=-(1 << 31), hi=1 << 31),
    "int64": dict(kind=0, ms=False, lo=-(1 << 62), hi=1 << 62),
    "int / float mixed": dict(kind=None, ms=False, lo=-(1 << 20), hi=1 << 20),
    "mixed widths": dict(kind=0, ms=None, lo=-300, hi=300),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("n", [1, 2, 9, 64, 513])
def test_facts_follow_from_the_encoder_inputs(name, n):
    c = CASES[name]
    rng = np.random.default_rng(n * 31 + len(name))
    sec = np.sort(rng.choice(3600, size=n, replace=False)).astype(np.int64)
    ms = np.full(n, bool(c["ms"])) if c["ms"] is not None else rng.random(n) < 0.5
    ts = T0 * 1000 + sec * 1000 + np.where(ms, rng.integers(1, 999, n), 0)
    kind = np.full(n, c["kind"]) if c["kind"] is not None else rng.integers(0, 3, n)
    lv = rng.integers(c.get("lo", 0), c.get("hi", 1), n)
    fv = rng.normal(0, 1e3, n)
    fv = np.where(kind == 1, fv.astype(np.float32).astype(np.float64), fv)
    if c.get("specials"):
        for i, s in zip(rng.choice(n, size=min(n, 4), replace=False), (np.nan, -0.0, np.inf, 1e-45)):
            fv[i] = np.float32(s)
    rows = synth.encode_rows(ts, lv, fv, kind, ms)
    assert len(rows) == 1
    f = R.row_facts(rows[0][1], rows[0][2])
    x = np.where(kind == 0, lv.astype(np.float64), fv)          # every value as the double a sum reads
    assert f.ndp == n and not f.err and not f.unsorted
    assert f.qw == (4 if ms.all() else 2 if not ms.any() else 0)
    assert f.allf == bool((kind != 0).all()) and f.alli == bool((kind == 0).all())
    L = np.where(kind == 1, 4, np.where(kind == 2, 8, synth.vle_lengths(lv)))
    assert f.vle2 == bool((L <= 2).all())
    assert f.vl == (int(L[0]) if f.qw and (L == L[0]).all() else 0)
    assert f.nan == bool(np.isnan(x).any())
    assert f.negz == bool(((x == 0) & np.signbit(x) & (kind != 0)).any())
    fin = x[~np.isnan(x)]
    assert f.absmax == (float(np.abs(fin).max()) if len(fin) else 0.0)
    nz = [v for v in fin.tolist() if v != 0.0 and not math.isinf(v)]
    assert f.lsb == (min(_lsb_of_inputs(v) for v in nz) if nz else INT32_MAX)
    assert f.first_ms == int(ts[0] - T0 * 1000) and f.max_ms == int(ts[-1] - T0 * 1000)


def test_unsorted_follows_from_the_inputs():
    """A swapped pair of qualifiers inside a cell; and across rows, a second row of the same hour
    (its first datapoint not after the first row's last), through index_ref's series walk."""
    q = q2(5, 0) + q2(3, 0) + q2(9, 0)
    assert R.row_facts(q, b"\x01\x02\x03\x00").unsorted
    assert R.row_facts(q2(3, 0) + q2(3, 0), b"\x01\x02\x00").unsorted          # equal offsets: not strictly increasing
    assert not R.row_facts(q2(3, 0) + q2(5, 0) + q2(9, 0), b"\x01\x02\x03\x00").unsorted
    assert R.row_facts(q4(2000, 0) + q4(1999, 0), b"\x01\x02\x00").unsorted
    assert R.row_facts(q2(2, 0) + q4(1999, 0), b"\x01\x02\x01").unsorted      # 2 s, then 1.999 s
    rows = [(T0, q2(10, 0) + q2(20, 0), b"\x01\x02\x00"), (T0, q2(20, 0), b"\x03"), (T0 + 3600, q2(0, 0), b"\x04"),
            (T0 + 3600, q2(1, 0), b"\x05")]
    b = synth.from_series([rows, rows[:1]], [0, 1])
    flags = R.index_ref(b)[1]
    assert [bool(f & R.ROW_UNSORTED) for f in flags] == [False, True, False, False, False]


F32 = 0xB
LITERALS = [
    # name, qualifiers, values, {fact: expected}
    ("float32 denormal 0x00000001", q2(0, F32), bytes.fromhex("00000001"),
     dict(ndp=1, qw=2, vl=4, allf=True, alli=False, vle2=False, lsb=-149, absmax=2.0 ** -149, nocert=False)),
    ("1.5f", q2(0, F32), bytes.fromhex("3fc00000"), dict(lsb=-1, absmax=1.5, allf=True, nocert=False)),
    ("int16 -32768", q2(0, 1), bytes.fromhex("8000"),
     dict(absmax=32768.0, lsb=15, alli=True, vle2=True, vl=2, nocert=False)),
    ("int32 INT32_MIN", q2(0, 3), bytes.fromhex("80000000"),
     dict(absmax=2147483648.0, lsb=31, alli=True, vle2=False, vl=4)),
    ("int8 -128 and 127", q2(0, 0) + q2(1, 0), bytes.fromhex("807f00"),
     dict(ndp=2, absmax=128.0, lsb=0, vl=1, vle2=True)),
    ("all zero", q2(0, 0) + q2(1, 1) + q2(2, F32), bytes.fromhex("00" "0000" "00000000" "00"),
     dict(ndp=3, lsb=INT32_MAX, absmax=0.0, nan=False, negz=False, nocert=False, vl=0, allf=False, alli=False)),
    ("NaN only", q2(0, F32) + q2(1, F32), bytes.fromhex("7fc00000" "ffc00001" "00"),
     dict(ndp=2, lsb=INT32_MAX, absmax=0.0, nan=True, negz=False, nocert=False)),
    ("-0.0 and +Inf", q2(0, F32) + q2(1, F32) + q2(2, F32), bytes.fromhex("80000000" "7f800000" "40000000" "00"),
     dict(negz=True, nan=False, absmax=math.inf, lsb=1, nocert=True)),
    ("-Inf in float64", q4(1, 0xF), bytes.fromhex("fff0000000000000"),
     dict(qw=4, vl=8, absmax=math.inf, lsb=INT32_MAX, nocert=False)),
    ("float64 2^53+2 beside 1.0", q2(0, 0xF) + q2(1, 0xF), bytes.fromhex("4340000000000001" "3ff0000000000000" "00"),
     dict(absmax=2.0 ** 53 + 2, lsb=0, nocert=True, vl=8)),
    ("float64 2^50 beside 1.0", q2(0, 0xF) + q2(1, 0xF), bytes.fromhex("4310000000000000" "3ff0000000000000" "00"),
     dict(absmax=2.0 ** 50, lsb=0, nocert=False)),
    ("float64 2^51 beside 1.0", q2(0, 0xF) + q2(1, 0xF), bytes.fromhex("4320000000000000" "3ff0000000000000" "00"),
     dict(absmax=2.0 ** 51, lsb=0, nocert=True)),   # two of them reach 2^52: the margin of row_nocert
    ("int64 2^53+1 rounds to 2^53", q2(0, 7), bytes.fromhex("0020000000000001"),
     dict(absmax=2.0 ** 53, lsb=53, alli=True, vl=8)),
    ("int64 INT64_MIN", q2(0, 7), bytes.fromhex("8000000000000000"), dict(absmax=2.0 ** 63, lsb=63)),
    ("mixed widths, uniform lengths", q2(1, 0) + q4(2500, 0), bytes.fromhex("060c01"),
     dict(ndp=2, qw=0, vl=0, alli=True, vle2=True, absmax=12.0, lsb=1, unsorted=False)),
    ("4-byte qualifiers, vle", q4(1, 0) + q4(2, 1), bytes.fromhex("03" "0100" "00"),
     dict(ndp=2, qw=4, vl=0, absmax=256.0, lsb=0, vle2=True)),
]


@pytest.mark.parametrize("name,q,v,want", LITERALS, ids=[c[0] for c in LITERALS])
def test_hand_written_cells(name, q, v, want):
    f = R.row_facts(q, v)
    assert not f.err
    got = {k: getattr(f, k) for k in want}
    assert got == want


def test_flag_word_layout():
    """The packed flags are engine.h's bits."""
    f = R.row_facts(q2(0, F32) + q2(1, F32) + q2(2, F32) + q2(3, F32),
                    bytes.fromhex("80000000" "7f800000" "7fc00000" "3f800000" "00"))
    assert f.flags() == 2 | (4 << 8) | 0x20000 | 0x40000 | 0x80000 | 0x1000000
    f = R.row_facts(q2(1, 0) + q2(0, 1), bytes.fromhex("01" "0002" "00"))
    assert f.flags() == 2 | 0x100000 | 0x400000 | 0x800000
    assert R.row_facts(q2(0, 2), b"\x00\x00\x01").flags() & 0x10000


@pytest.mark.parametrize("name,q,v,malformed", R.MALFORMED_CELLS, ids=[c[0] for c in R.MALFORMED_CELLS])
def test_err_is_what_the_oracle_refuses(name, q, v, malformed):
    """A raw sum over a batch holding only the cell raises IllegalDataException on the oracle
    exactly when the reference says ROW_ERR."""
    f = R.row_facts(q, v)
    assert f.err == malformed
    b = R.one_row_batch([(q, v)], T0)
    query = abi.new_query(T0, T0 + 3599, "sum")
    if malformed:
        with pytest.raises(O.OracleError) as ei:
            O.run_query(b, query)
        assert ei.value.code == abi.TSDB_E_ILLEGAL_DATA
    else:
        assert len(O.run_query(b, query)) == 1
