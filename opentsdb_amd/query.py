"""Host-side mirror of the reference query API for the aggregation path.

The Java host keeps these classes unchanged and binds libtsdbhip through JNI
(INTEGRATION.md).  No JDK exists in this pipeline, so this module restates the pieces
of them that feed the C ABI, with the same names, argument meaning and exceptions, so
the parity tests read like the reference's own tests:

  * TsdbQuery.setStartTime / setEndTime / setTimeSeries / downsample / run
      (src/core/TsdbQuery.java:262-319, 434-560, 716-1049)
  * DownsamplingSpecification(String)    (src/core/DownsamplingSpecification.java:116-191)
  * RateOptions                          (src/core/RateOptions.java:27-97)
  * DataPoints / DataPoint views of a result (src/core/DataPoints.java, DataPoint.java)

run() does what findSpans + GroupByAndAggregateCB do on the host (scan the store for
the metric, filter tags, group spans by the group-by tag values in ByteMap order) and
hands the flattened Spans to a runner -- libtsdbhip on the GPU by default.
"""
from __future__ import annotations

import struct
import time
from dataclasses import dataclass

import numpy as np

from . import abi
from .store import MockStore, _tag_bytes, make_batch

SECOND_MASK = 0xFFFFFFFF00000000


class QueryException(Exception):
    """A reference exception surfaced through the C ABI (Java class in .java)."""

    def __init__(self, code: int, msg: str = ""):
        self.code = code
        self.java = abi.ERROR_NAMES.get(code, str(code))
        super().__init__(f"{self.java}: {msg}")


@dataclass
class RateOptions:
    counter: bool = False
    counter_max: int = abi.LONG_MAX
    reset_value: int = 0
    drop_resets: bool = False


def parse_duration(duration: str) -> int:
    """DateTime.parseDuration (src/utils/DateTime.java:186-226)."""
    unit = 0
    while unit < len(duration) and duration[unit].isdigit():
        unit += 1
        if unit >= len(duration):
            raise ValueError(f"Invalid duration, must have an integer and unit: {duration}")
    if unit == 0:
        raise ValueError(f"Invalid duration (number): {duration}")
    interval = int(duration[:unit])
    if interval <= 0:
        raise ValueError(f"Zero or negative duration: {duration}")
    c = duration[-1].lower()
    if c == "s":
        if len(duration) >= 2 and duration[-2] == "m":
            return interval
        mult = 1
    else:
        mult = {"m": 60, "h": 3600, "d": 86400, "w": 604800, "n": 2592000, "y": 31536000}.get(c)
        if mult is None:
            raise ValueError(f"Invalid duration (suffix): {duration}")
    return interval * mult * 1000


@dataclass
class DownsamplingSpecification:
    """new DownsamplingSpecification(String) / (interval, function, fill)."""
    interval: int = 0
    function: str | None = None
    fill_policy: str = "none"
    run_all: bool = False
    use_calendar: bool = False
    calendar_unit: int = 0     # abi.CAL_* of a 'c' interval (DateTime.unitsToCalendarType)
    timezone: str | None = None   # setTimezone (DownsamplingSpecification.java:199-207); None = UTC

    def setTimezone(self, tz: str) -> None:
        if tz is None:
            raise ValueError("Timezone cannot be null")
        self.timezone = tz

    @classmethod
    def parse(cls, spec: str) -> "DownsamplingSpecification":
        parts = spec.split("-")
        while parts and parts[-1] == "":
            parts.pop()
        if len(parts) < 2:
            raise ValueError(f"Invalid downsampling specifier '{spec}': must provide at least interval and function")
        if len(parts) > 3:
            raise ValueError(f"Invalid downsampling specifier '{spec}': must consist of interval, function, and optional fill policy")
        ds = cls()
        if "all" in parts[0]:
            ds.run_all = True
        elif parts[0].endswith("c"):
            ds.interval = parse_duration(parts[0][:-1])
            ds.use_calendar = True
            d = parts[0][:-1]
            ds.calendar_unit = abi.CAL_MS if d.lower().endswith("ms") else \
                {"s": abi.CAL_S, "m": abi.CAL_M, "h": abi.CAL_H, "d": abi.CAL_D, "w": abi.CAL_W, "n": abi.CAL_N,
                 "y": abi.CAL_Y}[d[-1]]
        else:
            ds.interval = parse_duration(parts[0])
        if parts[1] not in abi.AGG:
            raise ValueError(f"No such downsampling function: {parts[1]}")
        if parts[1] == "none":
            raise ValueError("cannot use the NONE aggregator for downsampling")
        ds.function = parts[1]
        if len(parts) == 3:
            if parts[2].lower() not in abi.FILL_NAMES:
                raise ValueError(f"Unrecognized fill policy: {parts[2]}")
            ds.fill_policy = parts[2].lower()
        return ds


class DataPoint:
    __slots__ = ("_ts", "_int", "_v")

    def __init__(self, ts: int, is_int: bool, v):
        self._ts, self._int, self._v = ts, is_int, v

    def timestamp(self) -> int:
        return self._ts

    def isInteger(self) -> bool:
        return self._int

    def longValue(self) -> int:
        if not self._int:
            raise TypeError("ClassCastException: value is a double")
        return self._v

    def doubleValue(self) -> float:
        if self._int:
            raise TypeError("ClassCastException: value is a long")
        return self._v

    def toDouble(self) -> float:
        return float(self._v)


class DataPoints:
    """One SpanGroup's materialised output (arrays from tsdbhip_result)."""

    def __init__(self, group_id: int, ts: np.ndarray, bits: np.ndarray, is_int: np.ndarray,
                 metric: str = "", group_key: tuple = ()):
        self.group_id = group_id
        self.ts = np.asarray(ts, np.int64)
        self.bits = np.asarray(bits, np.uint64)
        self.is_int = np.asarray(is_int, np.uint8)
        self.metric = metric
        self.group_key = group_key

    def size(self) -> int:
        return len(self.ts)

    def timestamp(self, i: int) -> int:
        return int(self.ts[i])

    def isInteger(self, i: int) -> bool:
        return bool(self.is_int[i])

    def longValue(self, i: int) -> int:
        return int(self.bits[i].astype(np.int64))

    def doubleValue(self, i: int) -> float:
        return struct.unpack("<d", struct.pack("<Q", int(self.bits[i])))[0]

    def values(self) -> np.ndarray:
        """float64 view of every point (longs converted like toDouble())."""
        d = self.bits.view(np.float64).copy()
        ints = self.is_int.astype(bool)
        d[ints] = self.bits[ints].view(np.int64).astype(np.float64)
        return d

    def __iter__(self):
        for i in range(len(self.ts)):
            if self.is_int[i]:
                yield DataPoint(int(self.ts[i]), True, self.longValue(i))
            else:
                yield DataPoint(int(self.ts[i]), False, self.doubleValue(i))

    def metricName(self) -> str:
        return self.metric


FILTER_TYPES = ("literal_or", "iliteral_or", "not_literal_or", "not_iliteral_or", "wildcard", "iwildcard", "regexp", "not_key")


class TagVFilter:
    """One 2.x tag value filter (src/query/filter/TagV*Filter.java): its type, tagk, filter string
    and groupBy flag, with the reference's constructor checks and match(tags) over a
    {tagk name: tagv name} map."""

    def __init__(self, type: str, tagk: str, filter: str = "", group_by: bool = False):
        if type not in FILTER_TYPES:
            raise ValueError(f"Could not find a tag value filter of the type: {type}")
        if not tagk:
            raise ValueError("Filter must have a tagk")
        self.type, self.tagk, self.filter, self.group_by = type, tagk, filter or "", bool(group_by)
        self.case_insensitive = type in ("iliteral_or", "not_iliteral_or", "iwildcard")
        f = self.filter
        if type == "not_key":
            if f:
                raise ValueError("The filter must be empty for the not_key filter")
        elif not f:
            raise ValueError("Filter cannot be null or empty")
        if type.endswith("literal_or"):
            if len(f) == 1 and f == "|":
                raise ValueError("Filter must contain more than just a pipe")
            # Java's String.split drops the trailing empty strings
            parts = f.split("|")
            while parts and parts[-1] == "":
                parts.pop()
            self.literals = {p.lower() if self.case_insensitive else p for p in parts}
        elif type.endswith("wildcard"):
            actual = f.lower() if self.case_insensitive else f
            if "*" not in actual:
                raise ValueError("Filter must contain an asterisk")
            self.has_postfix = actual[0] == "*"
            while actual[0] == "*" and len(actual) >= 2:
                actual = actual[1:]
            self.has_prefix = actual[-1] == "*"
            while actual[-1] == "*" and len(actual) >= 2:
                actual = actual[:-1]
            self.components = actual.split("*") if actual.find("*") > 0 else [actual]
        elif type == "regexp":
            import re
            self.pattern = re.compile(f)

    @classmethod
    def of(cls, entry) -> "TagVFilter":
        """From a filter list entry: a TagVFilter, or a {"type", "tagk", "filter", "groupBy"} mapping."""
        if isinstance(entry, cls):
            return entry
        return cls(entry["type"], entry["tagk"], entry.get("filter", ""), entry.get("groupBy", False))

    def matches_all(self) -> bool:
        return self.type.endswith("wildcard") and self.components == ["*"]

    def match_value(self, tagv: str) -> bool:
        """The filter's verdict on a present tag value (the part of match after the null check)."""
        if self.type in ("literal_or", "iliteral_or"):
            return (tagv.lower() if self.case_insensitive else tagv) in self.literals
        if self.type in ("not_literal_or", "not_iliteral_or"):
            return (tagv.lower() if self.case_insensitive else tagv) not in self.literals
        if self.type == "regexp":
            return self.pattern.search(tagv) is not None
        if self.type == "not_key":
            return False
        if self.matches_all():
            return True
        if self.case_insensitive:
            tagv = tagv.lower()
        comps = self.components
        if self.has_postfix and not self.has_prefix and not tagv.endswith(comps[-1]):
            return False
        if self.has_prefix and not self.has_postfix and not tagv.startswith(comps[0]):
            return False
        idx = 0
        for c in comps:   # (the reference advances by the component's length, not to the match's end)
            if tagv.find(c, idx) < 0:
                return False
            idx += len(c)
        return True

    def match(self, tags: dict) -> bool:
        tagv = tags.get(self.tagk)
        if tagv is None:   # a missing tag: only the negated filters hold
            return self.type in ("not_literal_or", "not_iliteral_or", "not_key")
        return self.match_value(tagv)


UNSET = -1
ROLLUP_USAGES =("ROLLUP_RAW", "ROLLUP_NOFALLBACK", "ROLLUP_FALLBACK", "ROLLUP_FALLBACK_RAW")


class TsdbQuery:
    """Mirror of net.opentsdb.core.TsdbQuery for the aggregation path."""

    def __init__(self, store: MockStore, runner=None, rollups=None, rollup_runner=None, fix_duplicates=False):
        self.store = store
        self.runner = runner
        self.rollups = rollups              # rollup_read.RollupStore (tsdb.getRollupConfig() + tables)
        self.rollup_runner = rollup_runner  # (HostRollupBatch, Query) -> groups; libtsdbhip by default
        self.fix_duplicates = fix_duplicates
        self.start_time = UNSET
        self.end_time = UNSET
        self.metric = None
        self.tags = {}
        self.filters = []                   # setFilters: the 2.x TagVFilter list
        self.explicit_tags = False
        self.aggregator = None
        self.rate = False
        self.rate_options = RateOptions()
        self.downsampler: DownsamplingSpecification | None = None
        self.flags = 0
        self.rollup_usage = "ROLLUP_NOFALLBACK"   # TsdbQuery.java:150
        self.pre_aggregate = False                # TsdbQuery.java:154

    def setPreAggregate(self, pre_aggregate: bool = True):
        """TSSubQuery.setPreAggregate -> TsdbQuery.pre_aggregate (TsdbQuery.java:458): read the
        pre-aggregated (group-by) table instead of aggregating after the fetch."""
        self.pre_aggregate = bool(pre_aggregate)

    def isPreAggregate(self) -> bool:   # TsdbQuery.java:257-259
        return self.pre_aggregate

    def _agg_tag(self):
        """(tsdb.getAggTagKey(), tsdb.getRawTagValue()): tsd.rollups.agg_tag_key / raw_agg_tag_value."""
        if self.rollups is not None:
            return self.rollups.agg_tag_key, self.rollups.raw_agg_tag_value
        return "_aggregate", "RAW"

    def tableToBeScanned(self):
        """TsdbQuery.tableToBeScanned (:1484-1503) as (kind, rollup interval name | None):
        "rollup-agg" the matched interval's group-by table, "rollup" its temporal table, "agg" the
        default interval's group-by table, "raw" the data table."""
        name = self.rollup_interval_name()
        if name is not None:
            return ("rollup-agg" if self.pre_aggregate else "rollup"), name
        return ("agg" if self.pre_aggregate else "raw"), None

    def setRollupUsage(self, usage: str | None):
        """TSSubQuery.setRollupUsage / ROLLUP_USAGE.parse (TsdbQuery.java:207-222): an unknown
        name means ROLLUP_NOFALLBACK."""
        u = (usage or "").upper()
        self.rollup_usage = u if u in ROLLUP_USAGES else "ROLLUP_NOFALLBACK"

    # TsdbQuery.java:262-319
    def setStartTime(self, timestamp: int):
        if timestamp < 0 or ((timestamp & SECOND_MASK) != 0 and timestamp > 9999999999999):
            raise ValueError(f"Invalid timestamp: {timestamp}")
        if self.end_time != UNSET and timestamp >= self.getEndTime():
            raise ValueError(f"new start time ({timestamp}) is greater than or equal to end time")
        self.start_time = timestamp

    def setEndTime(self, timestamp: int):
        if timestamp < 0 or ((timestamp & SECOND_MASK) != 0 and timestamp > 9999999999999):
            raise ValueError(f"Invalid timestamp: {timestamp}")
        if self.start_time != UNSET and timestamp <= self.getStartTime():
            raise ValueError(f"new end time ({timestamp}) is less than or equal to start time")
        self.end_time = timestamp

    def getStartTime(self) -> int:
        if self.start_time == UNSET:
            raise RuntimeError("IllegalStateException: setStartTime was never called!")
        return self.start_time

    def getEndTime(self) -> int:
        if self.end_time == UNSET:
            self.setEndTime(int(time.time() * 1000))
        return self.end_time

    def setTimeSeries(self, metric: str, tags: dict, function: str, rate: bool,
                      rate_options: RateOptions | None = None):
        if function not in abi.AGG:
            raise KeyError(f"No such aggregator: {function}")
        self.metric = metric
        self.tags = dict(tags)
        self.aggregator = function
        self.rate = rate
        self.rate_options = rate_options or RateOptions()
        # a literal filter on the aggregate tag key asking for anything but the raw value reads
        # pre-aggregated data (TsdbQuery.java:565-571)
        agg_tag_key, raw_value = self._agg_tag()
        v = self.tags.get(agg_tag_key)
        if v is not None and "*" not in v and v != raw_value:
            self.pre_aggregate = True

    def downsample(self, interval, function: str | None = None, fill_policy: str = "none"):
        """downsample(interval_ms, Aggregator[, FillPolicy]) or downsample("1m-avg")."""
        if isinstance(interval, str):
            self.downsampler = DownsamplingSpecification.parse(interval)
            return
        if function is None:
            raise ValueError("downsampling function cannot be null")
        if interval <= 0:
            raise ValueError(f"interval not > 0: {interval}")
        if function == "none":
            raise ValueError("cannot use the NONE aggregator for downsampling")
        self.downsampler = DownsamplingSpecification(interval=interval, function=function,
                                                     fill_policy=fill_policy)

    def setOrdered(self, ordered: bool = True):
        """Engine option: cross-series float reductions in SpanGroup index order."""
        self.flags = (self.flags | abi.QF_ORDERED) if ordered else (self.flags & ~abi.QF_ORDERED)

    # -- C ABI structs -----------------------------------------------------------
    def to_abi(self) -> abi.Query:
        ds = self.downsampler
        q = abi.new_query(
            self.getStartTime(), self.getEndTime(), self.aggregator,
            ds_function=abi.AGG[ds.function] if ds else -1,
            ds_interval_ms=ds.interval if ds else 0,
            ds_fill=abi.FILL_NAMES.index(ds.fill_policy) if ds else abi.FILL_NONE,
            ds_all=bool(ds and ds.run_all), rate=self.rate, counter=self.rate_options.counter,
            counter_max=self.rate_options.counter_max, reset_value=self.rate_options.reset_value,
            drop_resets=self.rate_options.drop_resets, flags=self.flags)
        if ds and ds.use_calendar:
            q.ds_calendar = ds.calendar_unit
            if ds.timezone is not None:
                abi.set_timezone(q, ds.timezone)
        return q

    def scan_bounds(self):
        """getScanStartTimeSeconds / getScanEndTimeSeconds (TsdbQuery.java:1506-1606)."""
        start = self.getStartTime()
        if start & SECOND_MASK:
            start //= 1000
        ds = self.downsampler
        aligned = start
        if ds and ds.interval > 0:
            aligned -= ((1000 * start) % ds.interval) // 1000
        s = aligned - aligned % 3600
        s = s if s > 0 else 0
        end = self.getEndTime()
        if end & SECOND_MASK:
            end //= 1000
            if end - end * 1000 < 1:
                end += 1
        if ds and ds.interval > 0:
            ia = end + (ds.interval - (1000 * end) % ds.interval) // 1000
            off = ia % 3600
            e = ia if off == 0 else ia + (3600 - off)
        else:
            e = end + (3600 - end % 3600)
        return s, e

    def rollup_interval_name(self):
        """transformDownSamplerToRollupQuery (TsdbQuery.java:1665-1700): the best-match rollup
        table of the downsampling interval, or None (a raw scan) -- also when the best match is
        the default interval, the raw table itself (:1694-1697)."""
        best = self._best_rollups()
        if not best or self.rollups.config.isDefaultInterval(best[0]):
            return None
        return best[0]

    def setFilters(self, filters, explicit_tags: bool = False):
        """The 2.x filter list next to the old tags map (TSSubQuery.setFilters / setExplicitTags):
        TagVFilter objects or {"type", "tagk", "filter", "groupBy"} mappings, ANDed with each other
        and with setTimeSeries' tags.  explicit_tags: only series with exactly the filtered tag
        keys match (QueryUtil.getRowKeyUIDRegex without its skip-any-tags parts)."""
        self.filters = [TagVFilter.of(f) for f in filters]
        self.explicit_tags = bool(explicit_tags)

    def tag_query(self):
        """The query's tag filters and group-bys as data for tsdbhip_regroup_tags: an
        abi.HostTagQuery of filter primitives over UID sets, the group-by tagk uids of
        findGroupBys (TsdbQuery.java:613-706: a tagk is grouped when any of its filters has
        groupBy) and explicit_tags; None when no series can match (an unknown tag name, or an
        unknown literal of the old tags map: NoSuchUniqueName).  The old tags map goes through
        the same primitives: `*` is ANY plus group-by, `a|b` IN plus group-by, a literal IN.
        Wildcards, regular expressions and case-insensitive literals are resolved here over the
        tagv dictionary; every filter but not_key also asks for its tagk to be present, as the row
        key regex does for every row_key_literals entry (an ANY beside a NOT_IN)."""
        tagk_ids = self.store.tagk.ids
        tagv_ids = self.store.tagv.ids
        prims = []   # (tagk uid, abi.TF_*, ascending tagv uids)
        group_bys = set()
        for k, v in self.tags.items():
            if k not in tagk_ids:
                return None
            ku = tagk_ids[k]
            if v == "*":
                group_bys.add(ku)
                prims.append((ku, abi.TF_ANY, []))
            elif "|" in v:
                group_bys.add(ku)
                prims.append((ku, abi.TF_IN, sorted({tagv_ids[x] for x in v.split("|") if x in tagv_ids})))
            else:
                if v not in tagv_ids:
                    return None
                prims.append((ku, abi.TF_IN, [tagv_ids[v]]))
        for f in self.filters:
            if f.tagk not in tagk_ids:
                return None
            ku = tagk_ids[f.tagk]
            if f.group_by:
                group_bys.add(ku)
            if f.type == "not_key":
                prims.append((ku, abi.TF_NOT_KEY, []))
            elif f.matches_all():
                prims.append((ku, abi.TF_ANY, []))
            elif f.type in ("not_literal_or", "not_iliteral_or"):
                prims.append((ku, abi.TF_NOT_IN, sorted(u for name, u in tagv_ids.items() if not f.match_value(name))))
                prims.append((ku, abi.TF_ANY, []))
            else:
                prims.append((ku, abi.TF_IN, sorted(u for name, u in tagv_ids.items() if f.match_value(name))))
        return abi.HostTagQuery(prims, sorted(group_bys), self.explicit_tags)

    def _filters(self):
        """Tag filters and group-by tag uids of setTimeSeries' tags and setFilters' list (None: no
        series match): tag_query()'s primitives as a predicate over a series' (tagk, tagv) uids."""
        tq = self.tag_query()
        if tq is None:
            return None
        prims = [(ku, kind, set(vs)) for ku, kind, vs in tq.filter_list]
        wanted = sorted({ku for ku, kind, _ in prims if kind != abi.TF_NOT_KEY}) if tq.explicit_tags else None

        def pred(tags):
            d = dict(tags)
            for ku, kind, vs in prims:
                has = ku in d
                if kind == abi.TF_ANY:
                    ok = has
                elif kind == abi.TF_IN:
                    ok = has and d[ku] in vs
                elif kind == abi.TF_NOT_IN:
                    ok = not has or d[ku] not in vs
                else:
                    ok = not has
                if not ok:
                    return False
            return wanted is None or sorted(d) == wanted
        return pred, list(tq.group_by_list)

    @staticmethod
    def _groups(spans, group_bys):
        if not group_bys:
            return [()], [0] * len(spans)
        key_of = []
        for sk, _ in spans:
            d = dict(sk[1])
            key_of.append(tuple(d.get(ku, -1) for ku in group_bys))
        keys = sorted({k for k in key_of if -1 not in k})  # ByteMap order of the uid bytes
        index = {k: i for i, k in enumerate(keys)}
        return keys, [index.get(k, -1) for k in key_of]

    def build_rollup_batch(self, name: str):
        """The rollup scan of table `name` grouped like build_batch: (HostRollupBatch, keys)."""
        from .rollup_read import make_rollup_batch
        iv = self.rollups.config.intervals[name]
        f = self._filters()
        ds = self.downsampler
        if f is None:
            spans, need_count = [], False
        else:
            spans, need_count = self.rollups.scan_cells(name, self.metric, ds.function, self.aggregator, f[0],
                                                        groupby=self.pre_aggregate)
        keys, gids = self._groups(spans, f[1] if f else [])
        return make_rollup_batch(spans, gids, iv, need_count, self.fix_duplicates), keys

    def _data_store(self):
        """The table a query without a rollup match scans (tableToBeScanned :1495-1500): the data
        table, or for a pre-aggregate query the default interval's group-by table -- ordinary
        datapoint columns, so the ordinary batch path reads it."""
        if not self.pre_aggregate:
            return self.store
        if self.rollups is None:
            raise ValueError("a pre-aggregate query needs a rollup config (the default interval's group-by table)")
        return self.rollups.default_groupby

    def build_batch(self):
        """findSpans + GroupByAndAggregateCB grouping (TsdbQuery.java:795-1049).
        Returns (HostBatch, group keys in emission order)."""
        s, e = self.scan_bounds()
        f = self._filters()
        if f is None:   # an unknown tag name or literal value: no series matches
            return make_batch([], []), []
        pred, group_bys = f
        spans = self._data_store().scan(self.metric, s, e, pred)
        keys, gids = self._groups(spans, group_bys)
        return make_batch(spans, gids), keys

    def _best_rollups(self):
        """getRollupInterval's match list for the downsampling interval, best first ([] = none;
        ROLLUP_RAW never builds a rollup query, TsdbQuery.java:480-483)."""
        ds = self.downsampler
        if self.rollups is None or ds is None or ds.interval <= 0 or self.rollup_usage == "ROLLUP_RAW":
            return []
        from .rollup_read import NoSuchRollupForIntervalException
        try:
            return list(self.rollups.config.getRollupInterval(ds.interval // 1000))
        except NoSuchRollupForIntervalException:
            return []

    def _run_rollup(self, name):
        rb, keys = self.build_rollup_batch(name)
        q = self.to_abi()
        runner = self.rollup_runner
        if runner is None:
            from .engine import default_engine
            runner = default_engine().run_rollup_batch
        if rb.cells.n_series == 0:
            return []
        out = []
        for gid, ts, bits, isi in runner(rb, q):
            key = keys[gid] if (self.aggregator != "none" and 0 <= gid < len(keys)) else ()
            out.append(DataPoints(gid, ts, bits, isi, self.metric, key))
        return out

    def _run_raw(self, aggregator_override):
        batch, keys = self.build_batch()
        q = self.to_abi()
        if aggregator_override:
            q.aggregator = abi.AGG[aggregator_override]
        runner = self.runner
        if runner is None:
            from .engine import default_engine
            runner = default_engine().run_batch
        if batch.n_series == 0:
            return []
        groups = runner(batch, q)
        out = []
        for gid, ts, bits, isi in groups:
            key = keys[gid] if (self.aggregator != "none" and 0 <= gid < len(keys)) else ()
            out.append(DataPoints(gid, ts, bits, isi, self.metric, key))
        return out

    def _rollup_to_downsampler(self, name):
        """transformRollupQueryToDownSampler (TsdbQuery.java:1706-1717): the raw scan downsamples
        at the failed rollup table's interval with the rollup aggregator (zimsum / mimmax /
        mimmin read as sum / max / min, RollupQuery.java:69-80)."""
        from .rollup_read import normalize_agg
        ds = self.downsampler
        self.downsampler = DownsamplingSpecification(
            interval=self.rollups.config.intervals[name].interval_s * 1000,
            function=normalize_agg(ds.function), fill_policy=ds.fill_policy if ds else "zero")

    def run(self):
        """TsdbQuery.run(): DataPoints[] of the query (one per SpanGroup).  With a rollup config
        the downsampler becomes a rollup query on the best-match table
        (transformDownSamplerToRollupQuery, :1665-1700; a count group-by turns into sum there);
        the default interval is the raw table.  Under ROLLUP_FALLBACK / ROLLUP_FALLBACK_RAW an
        empty result re-runs on the next best match or on raw data
        (FallbackRollupOnEmptyResult, :1293-1354).  The query's downsampler is restored after."""
        best = self._best_rollups()
        if not best:
            return self._run_raw(None)
        override = "sum" if self.aggregator == "count" else None
        cur = best.pop(0)
        if self.rollups.config.isDefaultInterval(cur):
            return self._run_raw(override)
        saved = self.downsampler
        try:
            while True:
                out = self._run_rollup(cur)
                if out or self.rollup_usage not in ("ROLLUP_FALLBACK", "ROLLUP_FALLBACK_RAW"):
                    return out
                if self.rollup_usage == "ROLLUP_FALLBACK_RAW":
                    self._rollup_to_downsampler(cur)
                    return self._run_raw(override)
                if not best:
                    return []
                nxt = best.pop(0)
                if self.rollups.config.isDefaultInterval(nxt):
                    self._rollup_to_downsampler(cur)
                    return self._run_raw(override)
                # (the next table's interval divides the sample interval: the downsampler keeps
                # its interval, :1331-1340)
                cur = nxt
        finally:
            self.downsampler = saved


class LastPoint:
    """One answer of /api/query/last (IncomingDataPoint as Internal.GetLastDataPointCB fills it):
    the timestamp in ms, the value -- a Python int for a Java long, a float for a double; Java's
    toString rendering is the serializer's business -- and the series' TSUID as a hex string."""

    __slots__ = ("timestamp", "value", "tsuid")

    def __init__(self, timestamp: int, value, tsuid: str):
        self.timestamp = timestamp
        self.value = value
        self.tsuid = tsuid

    def __repr__(self):
        return f"LastPoint({self.timestamp}, {self.value!r}, {self.tsuid!r})"


class ResidentSpans:
    """Every span of one metric over [scan_start_s, scan_end_s), loaded once and kept in HBM;
    each query then only regroups the resident series (Engine.regroup, tsdbhip_regroup) instead
    of filtering, flattening and uploading a batch of its own as TsdbQuery.build_batch does.

    run(tsdb_query) answers a raw-table TsdbQuery over `store` whose scan range lies inside the
    resident one: the query's tag filters decide which resident spans are visible
    (abi.GROUP_EXCLUDED for the others) and its group-by tags number the visible ones, with the
    query's own _filters() / _groups() logic.  With device_tags the spans' tags are resident too
    (Engine.load_tags) and run() leaves filtering, key extraction and numbering to the device
    (Engine.regroup_tags, tsdbhip_regroup_tags) instead of walking every span's tags here."""

    def __init__(self, store: MockStore, metric: str, scan_start_s: int, scan_end_s: int, engine=None,
                 device_tags: bool = False):
        if scan_end_s <= scan_start_s:
            raise ValueError("empty resident scan range")
        self.store = store
        self.metric = metric
        self.scan_start_s = scan_start_s
        self.scan_end_s = scan_end_s
        if engine is None:
            from .engine import default_engine
            engine = default_engine()
        self.engine = engine
        self.spans = store.scan(metric, scan_start_s, scan_end_s)   # SpanCmp order, no filter
        self.span_keys = [sk for sk, _ in self.spans]
        # (loaded ungrouped: every run() regroups before it queries)
        self.engine.load(make_batch(self.spans, [abi.GROUP_NONE] * len(self.spans)))
        self.device_tags = bool(device_tags)
        if self.device_tags:
            self._load_tags()

    def _load_tags(self):
        """The resident tag table of span_keys (Engine.load_tags, tsdbhip_tags_load): at construction,
        and again after an edit that added or retired a series -- the engine drops its table then."""
        self.engine.load_tags(*abi.tag_table_arrays([sk[1] for sk in self.span_keys]))

    def group_ids(self, query: TsdbQuery):
        """(group id of every resident span for `query`, group keys in emission order)."""
        f = query._filters()
        if f is None:   # an unknown tag name or literal value: no series matches
            return [abi.GROUP_EXCLUDED] * len(self.spans), []
        pred, group_bys = f
        visible = [i for i, sk in enumerate(self.span_keys) if pred(sk[1])]
        keys, gids = TsdbQuery._groups([self.spans[i] for i in visible], group_bys)
        ids = [abi.GROUP_EXCLUDED] * len(self.spans)
        for i, g in zip(visible, gids):
            ids[i] = g
        return ids, keys

    @staticmethod
    def _span_order(keys):
        """Series keys of one metric in SpanCmp order, as MockStore.series lists them."""
        return sorted(keys, key=lambda k: _tag_bytes(k[1]))

    def extend(self, scan_end_s: int, rescan_from_s: int | None = None):
        """Move the resident range's end to scan_end_s without a reload (Engine.append,
        tsdbhip_append): rescan [rescan_from_s, scan_end_s) -- by default from the largest
        resident row base time, the live hour, whose row the store may have rewritten since --
        and hand the engine that delta.  A rescanned row replaces the resident row of the same
        base time; series the scan meets for the first time are inserted where SpanCmp order puts
        them, excluded until the next run() regroups.  Returns the engine's abi.AppendInfo."""
        if scan_end_s < self.scan_end_s:
            raise ValueError(f"the resident range ends at {self.scan_end_s}: it cannot shrink to {scan_end_s}")
        if rescan_from_s is None:
            rescan_from_s = max((rows[-1][0] for _, rows in self.spans if rows), default=self.scan_end_s)
        delta = self.store.scan(self.metric, rescan_from_s, scan_end_s)
        old = dict(zip(self.span_keys, self.spans))
        dkeys = {sk for sk, _ in delta}
        # SpanCmp order over the union of the keys: the store's own series order (a resident series
        # whose rows have all left the store keeps its place)
        merged_keys = self._span_order(set(old) | dkeys)
        index_of = {sk: i for i, sk in enumerate(merged_keys)}
        series_index = [index_of[sk] for sk, _ in delta]
        series_new = [sk not in old for sk, _ in delta]
        info = self.engine.append(make_batch(delta, [abi.GROUP_EXCLUDED] * len(delta)), series_index, series_new)
        drows = dict(delta)
        spans = []
        for sk in merged_keys:
            by_base = {r[0]: r for r in (old[sk][1] if sk in old else [])}
            by_base.update({r[0]: r for r in drows.get(sk, [])})   # the delta wins
            spans.append((sk, [by_base[b] for b in sorted(by_base)]))
        self.spans = spans
        self.span_keys = merged_keys
        self.scan_end_s = scan_end_s
        if self.device_tags and any(series_new):
            self._load_tags()
        return info

    def refresh(self, from_s: int, to_s: int | None = None, remove_missing: bool = False):
        """Bring rows the store has changed inside the resident range up to date without a reload
        (Engine.upsert, tsdbhip_upsert): rescan [from_s, to_s) -- to_s defaults to the range's end
        -- and hand the engine that delta.  A rescanned row replaces the resident row of the same
        base time wherever it sits in its series (late datapoints, a compacted or repaired row),
        any other is inserted by base time (a back-filled gap); series the scan meets for the
        first time are inserted as extend inserts them.  The resident range does not move.  An
        upsert cannot remove rows: a resident row inside the window that the rescan no longer
        returns needs a reload -- or remove_missing=True, which first removes those rows as
        single-row ranges (Engine.remove, tsdbhip_remove; their spans stay, row-less ones
        included: retire_empty).  Returns the engine's abi.UpsertInfo."""
        if to_s is None:
            to_s = self.scan_end_s
        if from_s < self.scan_start_s or to_s > self.scan_end_s or to_s <= from_s:
            raise ValueError(f"the window [{from_s}, {to_s}) is empty or outside the resident range "
                             f"[{self.scan_start_s}, {self.scan_end_s})")
        delta = self.store.scan(self.metric, from_s, to_s)
        drows = dict(delta)
        missing = []
        for i, (sk, rows) in enumerate(self.spans):
            got = {r[0] for r in drows.get(sk, [])}
            for r in rows:
                if from_s <= r[0] < to_s and r[0] not in got:
                    if not remove_missing:
                        raise ValueError(f"the resident row of base time {r[0]} is gone from the store: an upsert cannot "
                                         "remove rows, reload the resident spans")
                    missing.append((i, r[0], r[0] + 1))
        if missing:
            self.engine.remove(missing)
            gone = {(i, b) for i, b, _ in missing}
            self.spans = [(sk, [r for r in rows if (i, r[0]) not in gone]) for i, (sk, rows) in enumerate(self.spans)]
        old = dict(zip(self.span_keys, self.spans))
        # SpanCmp order over the union of the keys: the store's own series order (as extend)
        merged_keys = self._span_order(set(old) | set(drows))
        index_of = {sk: i for i, sk in enumerate(merged_keys)}
        series_index = [index_of[sk] for sk, _ in delta]
        series_new = [sk not in old for sk, _ in delta]
        info = self.engine.upsert(make_batch(delta, [abi.GROUP_EXCLUDED] * len(delta)), series_index, series_new)
        spans = []
        for sk in merged_keys:
            by_base = {r[0]: r for r in (old[sk][1] if sk in old else [])}
            by_base.update({r[0]: r for r in drows.get(sk, [])})   # the delta wins
            spans.append((sk, [by_base[b] for b in sorted(by_base)]))
        self.spans = spans
        self.span_keys = merged_keys
        if self.device_tags and any(series_new):
            self._load_tags()
        return info

    def put(self, points):
        """Datapoint writes (TSDB.addPoint / IncomingDataPoints.addPoint) that land in the store and
        in the resident batch at the store's own granularity (Engine.put, tsdbhip_put): points is
        [(tags, timestamp, kind, value), ...] in write order, kind abi.PUT_LONG / PUT_FLOAT /
        PUT_DOUBLE.  Every point is written into the store (add_long / add_float / add_double).
        The points of resident series whose row base lies inside the resident range then go to the
        engine in one call, with the store's fix_duplicates, and the touched spans' rows are taken
        from the store's compacted rows.  Hours touched by a series that is not resident yet, and
        every hour of the call when the engine refuses it with an IllegalDataException (a
        duplicate the store may have overwritten, a malformed resident cell, a row that failed its
        compaction at the load) or as not implemented (a cell whose offsets do not increase), fall
        back to refresh() over those hours -- a rescan and an upsert, which raises what the store's
        own read of such a row raises; the store holds the points by then, so after any exception
        the caller brings the spans up to date with refresh().  Points outside the resident range
        only reach the store.  Returns (abi.PutInfo or None, [abi.UpsertInfo of each fallback])."""
        from .engine import EngineError
        from .store import base_time_of
        add = {abi.PUT_LONG: self.store.add_long, abi.PUT_FLOAT: self.store.add_float, abi.PUT_DOUBLE: self.store.add_double}
        index_of = {sk: i for i, sk in enumerate(self.span_keys)}
        direct, touched, fallback = [], set(), set()
        for tags, ts, kind, value in points:
            add[kind](self.metric, ts, value, tags)
            sk = self.store._series_uids(self.metric, tags)
            base = base_time_of(ts)
            if not self.scan_start_s <= base < self.scan_end_s:
                continue
            if sk in index_of:
                direct.append((index_of[sk], ts, kind, value))
                touched.add((sk, base))
            else:
                fallback.add(base)
        info = None
        if direct:
            try:
                info = self.engine.put(direct, fix_duplicates=self.store.fix_duplicates)
            except EngineError as e:
                if e.code not in (abi.TSDB_E_ILLEGAL_DATA, abi.TSDB_E_NOT_IMPLEMENTED):
                    raise
                fallback |= {base for _, base in touched}
                touched = set()
        for sk, base in touched:
            if base in fallback:
                continue   # (the rescan below brings the row)
            i = index_of[sk]
            by_base = {r[0]: r for r in self.spans[i][1]}
            by_base[base] = (base,) + tuple(self.store.compact((sk[0], sk[1], base)))
            self.spans[i] = (sk, [by_base[b] for b in sorted(by_base)])
        upserts = [self.refresh(base, base + 3600) for base in sorted(fallback)]
        return info, upserts

    def trim(self, scan_start_s: int, pack_dead_pct: int = 50):
        """Move the resident range's start to scan_start_s without a reload (Engine.trim,
        tsdbhip_trim): the rows a scan of [scan_start_s, scan_end_s) no longer returns -- those
        with a base time below scan_start_s -- are evicted.  A span left without rows stays, as
        extend keeps row-less ones, so the series' indices keep their meaning.  The blobs are
        re-laid without their dead bytes once those reach pack_dead_pct per cent of the used
        bytes; the default of 50 is a policy that mirrors the reserve tsdbhip_append grows by
        (option APPEND_RESERVE), not a measured optimum.  Returns the engine's abi.TrimInfo."""
        if scan_start_s < self.scan_start_s:
            raise ValueError(f"the resident range starts at {self.scan_start_s}: it cannot grow back to {scan_start_s}")
        if scan_start_s >= self.scan_end_s:
            raise ValueError(f"the resident range ends at {self.scan_end_s}: a start of {scan_start_s} leaves it empty")
        info = self.engine.trim(scan_start_s, pack_dead_pct)
        self.spans = [(sk, [r for r in rows if r[0] >= scan_start_s]) for sk, rows in self.spans]
        self.scan_start_s = scan_start_s
        return info

    def delete(self, query: TsdbQuery, drop_empty: bool = False, pack_dead_pct: int = 50):
        """The delete query (TsdbQuery.setDelete(true)): `query` is answered as run answers it --
        the reference returns the data it deletes --, then every row its scan returned leaves the
        store (MockStore.delete_rows over the query's scan bounds and tag filter) and the
        resident batch (Engine.remove, tsdbhip_remove: one range per matching resident series).
        With drop_empty the spans left without rows are retired with their keys.  Returns
        (DataPoints[], abi.RemoveInfo)."""
        out = self.run(query)   # (run's range checks)
        s, e = query.scan_bounds()
        f = query._filters()
        if f is None:   # an unknown tag name or literal value: no series matches
            matching = []
        else:
            pred = f[0]
            matching = [i for i, sk in enumerate(self.span_keys) if pred(sk[1])]
            self.store.delete_rows(self.metric, s, e, pred)
        info, new_index = self.engine.remove([(i, s, e) for i in matching], drop_empty, pack_dead_pct)
        hit = set(matching)
        self.spans = [(sk, [r for r in rows if not (i in hit and s <= r[0] < e)]) for i, (sk, rows) in enumerate(self.spans)]
        if drop_empty:
            self._retire(new_index)
        return out, info

    def retire_empty(self):
        """Retire the spans without rows -- what trim, delete and refresh(remove_missing=True)
        left behind -- from the resident batch (Engine.remove with drop_empty and no range) and
        from spans / span_keys.  Returns the engine's abi.RemoveInfo."""
        info, new_index = self.engine.remove([], True)
        self._retire(new_index)
        return info

    def _retire(self, new_index):
        kept = [(sk, rows) for sk, rows in self.spans if rows]
        if [i for i, (_, rows) in enumerate(self.spans) if rows] != [i for i, x in enumerate(new_index) if x >= 0]:
            raise RuntimeError("the engine retired other series than the row-less spans")
        self.spans = kept
        self.span_keys = [sk for sk, _ in kept]
        if self.device_tags and any(x < 0 for x in new_index):
            self._load_tags()

    @staticmethod
    def tsuid_of(series_key) -> str:
        """UniqueId.uidToString of a series key's TSUID: metric uid, then (tagk uid, tagv uid) pairs."""
        m, tags = series_key
        return (m.to_bytes(3, "big") + _tag_bytes(tags)).hex().upper()

    def last(self, sub_queries, back_scan: int = 0, now_s: int | None = None, last_write_s=None):
        """/api/query/last over the resident spans (QueryRpc.handleLastDataPointQuery): the newest
        datapoint of every series the sub-queries name, by one Engine.last call (tsdbhip_last).
        A sub-query is a mapping with "tsuids" (hex strings) or "metric" and exact "tags"; TSUIDs
        win when both are given.  Every series is anchored at now_s (default: the clock) and looked
        for over back_scan hour rows back from there -- or, with back_scan == 0 and last_write_s, a
        map TSUID -> the meta table's last-write time in seconds, each at its own time, a series the
        map does not hold having no answer (TSUIDQuery.getLastPoint's meta path).  Returns the
        LastPoints in sub-query order with the nulls dropped, as FetchCB drops them; an unknown
        TSUID, tag name or tag combination yields none.  A metric other than the resident one
        raises ValueError, like run."""
        if back_scan < 0:
            raise ValueError("Backscan must be zero or a positive number")   # TSUIDQuery.getLastPoint
        if now_s is None:
            import time
            now_s = int(time.time())
        index_of = {self.tsuid_of(sk): i for i, sk in enumerate(self.span_keys)}
        wanted = []   # TSUIDs in answer order; None: no such series
        for sub in sub_queries:
            if sub.get("tsuids"):
                wanted += [t.upper() if t.upper() in index_of else None for t in sub["tsuids"]]
                continue
            if sub.get("metric") != self.metric:
                raise ValueError("the sub-query is over another metric than the resident spans")
            try:
                tags = tuple(sorted((self.store.tagk.ids[k], self.store.tagv.ids[v]) for k, v in (sub.get("tags") or {}).items()))
                t = self.tsuid_of((self.store.metrics.ids[self.metric], tags))
            except KeyError:   # NoSuchUniqueName
                t = None
            wanted.append(t if t in index_of else None)
        each = back_scan == 0 and last_write_s is not None
        if each:
            last_write_s = {k.upper(): v for k, v in last_write_s.items()}
            wanted = [t if t in last_write_s else None for t in wanted]
        asked = [t for t in wanted if t is not None]
        if not asked:
            return []
        ts, bits, kind, _ = self.engine.last([index_of[t] for t in asked], anchor_s=now_s,
                                             anchor_each=[int(last_write_s[t]) for t in asked] if each else None,
                                             back_scan=back_scan)
        out = []
        for t, ms, b, k in zip(asked, ts, bits, kind):
            if k == abi.LAST_INT:
                out.append(LastPoint(int(ms), int(np.uint64(b).astype(np.int64)), t))
            elif k == abi.LAST_FLOAT:
                out.append(LastPoint(int(ms), float(np.uint64(b).view(np.float64)), t))
        return out

    def run(self, query: TsdbQuery):
        """DataPoints[] of the query, keyed as TsdbQuery._run_raw keys them."""
        if query.store is not self.store or query.metric != self.metric:
            raise ValueError("the query is over another store or metric than the resident spans")
        if query.tableToBeScanned()[0] != "raw":
            raise ValueError("the resident spans answer raw-table queries only")
        s, e = query.scan_bounds()
        if s < self.scan_start_s or e > self.scan_end_s:
            raise ValueError(f"the query scans [{s}, {e}), outside the resident range "
                             f"[{self.scan_start_s}, {self.scan_end_s})")
        if self.device_tags:
            if not self.spans:
                return []
            tq = query.tag_query()
            if tq is None:   # an unknown tag name or literal value: no series matches
                keys = []
                self.engine.regroup([abi.GROUP_EXCLUDED] * len(self.spans))
            else:
                _, keys, _ = self.engine.regroup_tags(tq)
        else:
            ids, keys = self.group_ids(query)
            if not self.spans:
                return []
            self.engine.regroup(ids)
        out = []
        for gid, ts, bits, isi in self.engine.run(query.to_abi()):
            key = keys[gid] if (query.aggregator != "none" and 0 <= gid < len(keys)) else ()
            out.append(DataPoints(gid, ts, bits, isi, query.metric, key))
        return out
