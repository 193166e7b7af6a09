"""Host-side expectation of tsdbhip_put, never taken from the engine: put_batch gives the batch a
fresh load would be handed after the put, from the store's own encoders (opentsdb_amd.store) and
the oracle's CompactionQueue (oracle.compact_row) over [(resident qualifier, value)] + the puts as
single-datapoint columns with KeyValue timestamps 0, 1, 2, ...; store_rows builds the compacted
rows of a point list through MockStore, the second opinion of tests/test_put_cpu.py.

A point is (series_index, timestamp, kind, value): abi.make_points' tuple, kind abi.PUT_*."""
from __future__ import annotations

import numpy as np

from opentsdb_amd import abi, store, synth
from oracle import oracle as O
from tests.append_util import merge_batches, rows_of

L, F, D = abi.PUT_LONG, abi.PUT_FLOAT, abi.PUT_DOUBLE
ENCODE = {L: store.encode_long, F: store.encode_float, D: store.encode_double}


def encode(ts, kind, value):
    """(row base, qualifier bytes, value bytes) of one put."""
    v, flags = ENCODE[kind](value)
    return store.base_time_of(ts), store.build_qualifier(ts, flags), v


def bucket(points):
    """{(series, base): [(qualifier, value), ...] in write order}, identical qualifiers collapsed to
    the last one (an HBase cell version), and the number of points that collapse shadowed."""
    rows, shadowed = {}, 0
    for s, ts, kind, value in points:
        base, q, v = encode(ts, kind, value)
        cols = rows.setdefault((int(s), base), {})
        if q in cols:
            shadowed += 1
            del cols[q]          # (a dict keeps insertion order: the survivor takes the later place)
        cols[q] = v
    return {k: list(c.items()) for k, c in rows.items()}, shadowed


class PutExpectation:
    def __init__(self, batch, shadowed, added, rewritten):
        self.batch, self.shadowed, self.added, self.rewritten = batch, shadowed, added, rewritten


def put_batch(a, points, fix=False):
    """The host batch after tsdbhip_put(points) onto `a`, as a PutExpectation; or the OracleError
    code of the first touched row (in (series, base) order) whose compaction throws."""
    rows, shadowed = bucket(points)
    resident = [{b: (q, v) for b, q, v in rows_of(a, s)} for s in range(a.n_series)]
    delta, added = {}, 0
    for (s, base) in sorted(rows):
        assert 0 <= s < a.n_series, "a put names a resident series"
        cols = list(rows[(s, base)])
        if base in resident[s]:
            cols.insert(0, resident[s][base])
        else:
            added += 1
        try:
            q, v = O.compact_row(cols, fix, timestamps=list(range(len(cols))))
        except O.OracleError as e:
            return e.code
        delta.setdefault(s, []).append((base, q, v))
    idx = sorted(delta)
    d = synth.from_series([delta[s] for s in idx], [0] * len(idx))
    m = merge_batches(a, d, idx, [0] * len(idx)) if idx else a
    return PutExpectation(m, shadowed, added, len(rows) - added)


def store_rows(points, fix=False):
    """[(base, qualifier, value)] of one series' (timestamp, kind, value) writes, in write order,
    as a scan of a MockStore reads them (IllegalDataException when it throws)."""
    st = store.MockStore(fix_duplicates=fix)
    add = {L: st.add_long, F: st.add_float, D: st.add_double}
    for ts, kind, value in points:
        add[kind]("m", ts, value, {"h": "a"})
    spans = st.scan("m", 0, 1 << 40)
    return spans[0][1] if spans else []


def store_batch(series_points, gids, fix=False):
    """HostBatch of a store holding series_points[i] (write order) as series i."""
    return synth.from_series([store_rows(p, fix) for p in series_points], gids)
