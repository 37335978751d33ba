"""Aggregations around the device tables (slg_batch_prepare_aggs): request -> slg_agg_spec, tables -> response.

The device returns raw dense tables per node (PreparedBatch.aggs()).  Everything after the tables is host
work and lives here, a restatement of the reference's finish / finalize steps (query/aggs/mod.rs):
terms buckets ordered by count descending, then key STRING ascending (terms_bucket_cmp, :2469-2478), `size`
and `min_doc_count` (default 1); histogram keys id * interval + offset, `min_doc_count` (default 0 with
bounds, else 1), zero buckets over extended_bounds (or hard_bounds), ascending; range buckets in request order
with their key string or {"from", "to"}; stats with avg = sum / count (0.0 when empty); cardinality {"value": n};
percentiles and percentile_ranks {"values": {key: f64}} keyed by the percent / target as Rust's `format!("{p}")`
prints an f64 (:3245-3262), percentiles interpolated as QuantileState::percentile does (:529-537) — over ALL
values: the device is exact at any n, where the reference switches to a t-digest estimate above 256 values.
date_histogram keys are integers, bucket start + offset, ascending, `min_doc_count` (default 0), zero buckets walked
from bucket_start(min) to bucket_start(max) of extended_bounds (or hard_bounds) with add_interval
(DateHistogramCollector::finish, :1364-1403); filter {"doc_count", "aggregations"} (:2707-2726).  Two types are host
mappings onto device kinds: date_range is a range node whose bounds and `missing` went through parse_date
(DateRangeCollector, :1063-1122), value_count is the count of a stats node (ValueCountCollector, :1455-1476).

A request is the reference's `aggs` map: name -> {"type": "terms" | "histogram" | "range" | "stats" | "cardinality"
| "percentiles" | "percentile_ranks" | "date_histogram" | "date_range" | "filter" | "value_count", "field": ..., ...,
"aggs": {...children...}}.  Maps are walked in name order, as the reference's BTreeMaps.

top_hits ({"type": "top_hits", "size", "from", "sort": [{"field", "order"}]}, at the root or as a child of a root
bucket aggregation) travels beside the aggregation spec (slg_batch_prepare_top_hits): AggPlan.top_hits.  The device
returns (segment, doc, score) per hit; `fields` and `snippet` of the reference's TopHit are doc-store work on the
finished hits and are left out here.  The device keeps ONE list over all segments and reports its rows [from, from +
size); the reference slices every segment's list at `from` and the merged list again (TopHitsCollector::finish,
merge_top_hits), so with from > 0 and hits in more than one segment it answers differently: such a request is exact
on the device only when one segment holds the list's hits.

composite ({"type": "composite", "sources": [{"type": "terms" | "histogram", "name", "field", "interval"}], "size",
"after", "aggs"}, at the root, one per request) travels beside the aggregation spec too (slg_batch_prepare_composite):
AggPlan.composite.  The device returns the `size` smallest packed keys at or above a lower bound with their counts and
children; composite_lower_bound maps the request's `after` object to that bound, shape_composite renders the page
(CompositeCollector / finalize_composite, :1689-1842, :3264-3368).

significant_terms and rare_terms ({"type": "significant_terms", "field", "size", "min_doc_count", "background_filter",
"aggs"} / {"type": "rare_terms", "field", "size", "max_doc_count", "aggs"}, at the root, up to four per request)
travel beside the aggregation spec as well (slg_batch_prepare_term_buckets): AggPlan.term_buckets.  The device returns
at most `size` rows per node in the response's order; shape_term_buckets renders them (SignificantTermsCollector,
RareTermsCollector and finalize, :131-359, :2515-2595).  A background_filter is named through fields[FILTERS], as a
filter aggregation's filter.  The device counts over all segments before it applies the count bound and `size`, where
the reference does both per segment first.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import re
from typing import Dict, List, Optional

import numpy as np

from . import _native as N

KINDS = {"terms": N.AGG_TERMS, "histogram": N.AGG_HISTOGRAM, "range": N.AGG_RANGE, "stats": N.AGG_STATS,
         "cardinality": N.AGG_CARDINALITY, "percentiles": N.AGG_PERCENTILES, "percentile_ranks": N.AGG_PERCENTILE_RANKS,
         "date_histogram": N.AGG_DATE_HISTOGRAM, "filter": N.AGG_FILTER,
         "date_range": N.AGG_RANGE, "value_count": N.AGG_STATS}  # (the last two: host mappings)
BUCKET_TYPES = ("terms", "histogram", "range", "date_histogram", "date_range", "filter")
FILTERS = "$filters"  # the entry of `fields` that maps a filter aggregation's `filter` body to a registered filter id
DEFAULT_PERCENTS = [1.0, 5.0, 25.0, 50.0, 75.0, 95.0, 99.0]  # default_percentiles_list (:3376-3378)


def rust_f64(x: float) -> str:
    """format!("{x}") of an f64: the shortest digits that round-trip, never an exponent, and no ".0" on a whole
    number (50.0 -> "50", 99.9 -> "99.9", 1e21 -> "1000000000000000000000", -0.0 -> "-0")."""
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    r = repr(x)
    if "e" in r or "E" in r:
        from decimal import Decimal
        r = format(Decimal(r), "f")
    if r.endswith(".0"):
        r = r[:-2]
    return r


def node_percents(body: dict) -> List[float]:
    """the percents of a percentiles body (default list when absent) / the targets of a percentile_ranks body"""
    if body["type"] == "percentiles":
        return [float(p) for p in (body["percents"] if body.get("percents") is not None else DEFAULT_PERCENTS)]
    return [float(v) for v in body["values"]]


def percentile_of(n: int, low_bits: int, high_bits: int, pct: float) -> float:
    """QuantileState::percentile (:522-537) from the device's cells: n, the bits of vals[low] and vals[high]"""
    if n == 0:
        return 0.0
    lo = float(np.uint64(low_bits).view(np.float64))
    hi = float(np.uint64(high_bits).view(np.float64))
    rank = max((min(max(float(pct), 0.0), 100.0) / 100.0) * (float(n) - 1.0), 0.0)
    low, high = math.floor(rank), math.ceil(rank)
    if low == high:
        return lo
    w = rank - float(low)
    return lo * (1.0 - w) + hi * w


# ---- dates: parse_interval_seconds, parse_calendar_interval, parse_date, bucket_start, add_interval -------------
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
DAY_MS = 86_400_000
CALENDAR_UNITS = {"day": N.DATE_DAY, "1d": N.DATE_DAY, "week": N.DATE_WEEK, "1w": N.DATE_WEEK,
                  "month": N.DATE_MONTH, "1m": N.DATE_MONTH, "quarter": N.DATE_QUARTER, "1q": N.DATE_QUARTER,
                  "year": N.DATE_YEAR, "1y": N.DATE_YEAR}
_INTERVAL_UNITS = {"": 1.0, "s": 1.0, "ms": 0.001, "m": 60.0, "h": 3600.0, "d": 86_400.0, "w": 604_800.0}
_RUST_F64 = re.compile(r"[+-]?(?:(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?|(?i:inf|infinity|nan))\Z")
_RFC3339 = re.compile(r"(\d{4})-(\d\d)-(\d\d)[Tt ](\d\d):(\d\d):(\d\d)(?:\.(\d+))?([Zz]|[+-]\d\d:\d\d)\Z")


def rust_as_i64(x: float) -> int:
    """`x as i64`: truncation toward zero, saturating, NaN -> 0"""
    if math.isnan(x):
        return 0
    if math.isinf(x):
        return I64_MAX if x > 0 else I64_MIN
    return min(max(int(x), I64_MIN), I64_MAX)


def rust_parse_f64(s: str) -> Optional[float]:
    """`s.parse::<f64>().ok()`: no blanks, no underscores"""
    return float(s) if isinstance(s, str) and _RUST_F64.match(s) else None


def parse_interval_seconds(spec: str) -> Optional[float]:
    """:3474-3498: a prefix of ASCII digits and dots, then "", s, ms, m, h, d or w"""
    idx = 0
    while idx < len(spec) and (spec[idx] in "0123456789."):
        idx += 1
    if idx == 0:
        return None
    value = rust_parse_f64(spec[:idx])
    if value is None or spec[idx:] not in _INTERVAL_UNITS:
        return None
    return value * _INTERVAL_UNITS[spec[idx:]]


def parse_calendar_interval(spec: str) -> Optional[int]:
    """:3380-3389 -> DATE_DAY .. DATE_YEAR ("1m" is a month)"""
    return CALENDAR_UNITS.get("".join(c.lower() if c.isascii() else c for c in spec))


def days_from_civil(y: int, m: int, d: int) -> int:
    """days since 1970-01-01 of a proleptic-Gregorian date"""
    y -= m <= 2
    era = y // 400
    yoe = y - era * 400
    doy = (153 * (m + (-3 if m > 2 else 9)) + 2) // 5 + d - 1
    return era * 146097 + yoe * 365 + yoe // 4 - yoe // 100 + doy - 719468


def civil_from_days(z: int):
    """-> (y, m, d), the inverse of days_from_civil"""
    z += 719468
    era = z // 146097
    doe = z - era * 146097
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    d = doy - (153 * mp + 2) // 5 + 1
    m = mp + 3 if mp < 10 else mp - 9
    return yoe + era * 400 + (m <= 2), m, d


def _days_in_month(y: int, m: int) -> int:
    return days_from_civil(y + (m == 12), m % 12 + 1, 1) - days_from_civil(y, m, 1)


def parse_date(value) -> Optional[float]:
    """:3467-3472: RFC 3339 -> timestamp_millis() as f64, else a plain number"""
    if not isinstance(value, str):
        return None
    mt = _RFC3339.match(value)
    if mt:
        y, mo, d, h, mi, sec = (int(g) for g in mt.groups()[:6])
        if 1 <= mo <= 12 and 1 <= d <= _days_in_month(y, mo) and h < 24 and mi < 60 and sec < 60:
            ms = int((mt.group(7) or "0")[:3].ljust(3, "0"))
            tz = mt.group(8)
            shift = 0 if tz in "Zz" else (1 if tz[0] == "+" else -1) * (int(tz[1:3]) * 60 + int(tz[4:6])) * 60_000
            return float((days_from_civil(y, mo, d) * 86_400 + h * 3600 + mi * 60 + sec) * 1000 + ms - shift)
    return rust_parse_f64(value)


def bucket_start(value: int, offset: int, unit: int, step: int) -> int:
    """:3391-3401 with truncate_calendar (:3410-3429)"""
    t = value - offset
    if unit == N.DATE_FIXED:
        bucket = rust_as_i64(float(math.ceil(float(t) / float(step))))
        return min(max(bucket * step, I64_MIN), I64_MAX) + offset
    day = t // DAY_MS
    if unit == N.DATE_WEEK:
        day -= (day + 3) % 7  # (1970-01-01 was a Thursday)
    elif unit != N.DATE_DAY:
        y, m, _ = civil_from_days(day)
        m = 1 if unit == N.DATE_YEAR else (m - 1) // 3 * 3 + 1 if unit == N.DATE_QUARTER else m
        day = days_from_civil(y, m, 1)
    return day * DAY_MS + offset


def bucket_key(bucket_id: int, offset: int, unit: int, step: int) -> int:
    """the key of a device row: the start of bucket `bucket_id` (slg_date.hpp) + offset"""
    if unit == N.DATE_FIXED:
        return bucket_id * step + offset
    if unit == N.DATE_DAY:
        return bucket_id * DAY_MS + offset
    if unit == N.DATE_WEEK:
        return (7 * bucket_id - 3) * DAY_MS + offset
    month = bucket_id * {N.DATE_MONTH: 1, N.DATE_QUARTER: 3, N.DATE_YEAR: 12}[unit]
    return days_from_civil(1970 + month // 12, month % 12 + 1, 1) * DAY_MS + offset


def add_interval(current: int, unit: int, step: int) -> Optional[int]:
    """:3403-3465.  add_calendar re-truncates to midnight: a zero bucket behind the first loses a non-zero offset.
    None where chrono finds no such date (with_year / with_month keep the day of the month)."""
    if unit == N.DATE_FIXED:
        nxt = current + step
        return nxt if nxt <= I64_MAX else None
    day = current // DAY_MS
    if unit in (N.DATE_DAY, N.DATE_WEEK):
        return (day + (1 if unit == N.DATE_DAY else 7)) * DAY_MS
    y, m, d = civil_from_days(day)
    y2, m2 = y, m
    if unit == N.DATE_MONTH:
        m2 += 1
        if m2 > 12:
            y2, m2 = y + 1, 1
    elif unit == N.DATE_QUARTER:
        m2 += 3
        if m2 > 12:
            y2, m2 = y + 1, m2 - 12
    else:
        y2, m2 = y + 1, 1
    if d > _days_in_month(y2, m) or d > _days_in_month(y2, m2):  # with_year(y2)?.with_month(m2)?
        return None
    return days_from_civil(y2, m2, 1) * DAY_MS


def date_histogram_config(name: str, body: dict) -> dict:
    """DateHistogramCollector::new (:1264-1314) behind the request checks of validate_date_histogram_config
    (api/reader.rs:3877-...): -> dict(unit, step, offset, extended, hard, missing), times as i64 ms"""
    cal, fixed, off = body.get("calendar_interval"), body.get("fixed_interval"), body.get("offset")
    if cal is None and fixed is None:
        raise ValueError(f"date_histogram `{name}` requires `calendar_interval` or `fixed_interval`")
    if cal is not None and parse_calendar_interval(cal) is None:
        raise ValueError(f"date_histogram `{name}` calendar_interval `{cal}` is not supported")
    if fixed is not None and parse_interval_seconds(fixed) is None:
        raise ValueError(f"date_histogram `{name}` fixed_interval `{fixed}` is invalid")
    if off is not None and parse_interval_seconds(off) is None:
        raise ValueError(f"date_histogram `{name}` offset `{off}` is invalid")
    bounds = {}
    for which in ("extended_bounds", "hard_bounds"):
        b = body.get(which)
        if b is None:
            bounds[which] = None
            continue
        lo, hi = parse_date(b["min"]), parse_date(b["max"])
        for end, v in (("min", lo), ("max", hi)):
            if v is None:
                raise ValueError(f"date_histogram `{name}` {which}.{end} `{b[end]}` is not a valid date/number")
        if lo > hi:
            raise ValueError(f"date_histogram `{name}` {which}.min > max")
        bounds[which] = (rust_as_i64(lo), rust_as_i64(hi))
    if cal is not None:  # (calendar wins when both are given)
        unit, step = parse_calendar_interval(cal), 0
    else:
        unit, step = N.DATE_FIXED, rust_as_i64(parse_interval_seconds(fixed) * 1000.0)
    missing = body.get("missing")
    if isinstance(missing, (int, float)) and not isinstance(missing, bool):
        missing = float(missing)
    else:
        missing = parse_date(missing)  # (parse_date(s).or_else(|| s.parse::<f64>()): None when neither reads it)
    return dict(unit=unit, step=step, offset=0 if off is None else rust_as_i64(parse_interval_seconds(off) * 1000.0),
                extended=bounds["extended_bounds"], hard=bounds["hard_bounds"],
                missing=None if missing is None else rust_as_i64(missing))


def date_range_config(body: dict) -> dict:
    """DateRangeCollector::new (:1064-1094): -> dict(ranges=[(key, from, to)], missing), f64 or None (a bound that
    parse_date does not read is no bound)"""
    as_str = lambda v: v if v is None or isinstance(v, str) else json.dumps(v)
    ranges = [(rg.get("key"), None if rg.get("from") is None else parse_date(as_str(rg["from"])),
               None if rg.get("to") is None else parse_date(as_str(rg["to"]))) for rg in body["ranges"]]
    missing = body.get("missing")
    if isinstance(missing, str):
        missing = parse_date(missing)
    elif isinstance(missing, (int, float)) and not isinstance(missing, bool):
        missing = float(missing)
    else:
        missing = None
    return dict(ranges=ranges, missing=missing)


STATS_DTYPE = np.dtype([("count", np.uint64), ("min", np.float64), ("max", np.float64), ("sum", np.float64)])


class AggPlan:
    """A request's aggregations as the device takes them: .spec (N.AggSpec) and, per node in spec order,
    .nodes[i] = dict(name, type, body, parent, keys) for shape(); a date_histogram node also has date =
    date_histogram_config(), a date_range node date_range = date_range_config(), a filter node filter = its id.
    .top_hits is the N.TopHitsSpec of the request's top_hits nodes (None without one) and .top_hits_nodes[j] =
    dict(name, parent, from, size, sort) per node in its order, parent = -1 or the index in .nodes of its bucket
    aggregation, sort = [(sort field id or "_score", "asc" | "desc")]."""

    def __init__(self, spec: "N.AggSpec", nodes: List[dict], top_hits: Optional["N.TopHitsSpec"] = None,
                 top_hits_nodes: Optional[List[dict]] = None, composite: Optional[dict] = None,
                 term_buckets: Optional[dict] = None):
        self.spec = spec
        # the request's significant_terms / rare_terms aggregations (None without one): dict(spec = N.TermBucketSpec,
        # nodes = [dict(name, type, body, field, size, keys, rank, children = the AggPlan of its `aggs`)])
        self.term_buckets = term_buckets
        self.nodes = nodes
        self.top_hits = top_hits
        self.top_hits_nodes = top_hits_nodes or []
        # the request's composite aggregation (None without one): dict(name, body, spec = N.CompositeSpec, size, after,
        # sources = [dict(name, type, field, interval, keys, rank, sorted_keys)], children = the AggPlan of its `aggs`);
        # rank[ord] is the rank of ordinal ord's key in UTF-8 byte order (None: a histogram source), sorted_keys its
        # inverse as the key strings in that order
        self.composite = composite


VALUE_TYPES = ("cardinality", "percentiles", "percentile_ranks")


def _composite_plan(name: str, body: dict, fields: Dict[str, dict]) -> dict:
    """one composite body -> AggPlan.composite; ValueError for what the device does not build"""
    if body.get("sampling") is not None:
        raise ValueError(f"aggregation {name!r}: sampling is not built on the device")
    if body.get("size") is None:
        raise ValueError(f"aggregation {name!r}: composite requires `size`")
    size = int(body["size"])
    if size <= 0 or size > N.MAX_COMPOSITE_SIZE:
        raise ValueError(f"aggregation {name!r}: composite size {size} is not built on the device "
                         f"(1 .. {N.MAX_COMPOSITE_SIZE})")
    srcs = body.get("sources") or []
    if not 1 <= len(srcs) <= N.MAX_COMPOSITE_SOURCES:
        raise ValueError(f"aggregation {name!r}: a composite of {len(srcs)} sources is not built on the device")
    spec = N.CompositeSpec()
    spec.n_sources, spec.size = len(srcs), size
    sources = []
    for i, sb in enumerate(srcs):
        typ = sb.get("type")
        if typ not in ("terms", "histogram"):
            raise ValueError(f"aggregation {name!r}: composite source type {typ!r} is not built on the device")
        if sb["field"] not in fields or sb["field"] == FILTERS:
            raise ValueError(f"aggregation {name!r}: field {sb['field']!r} is not registered")
        fd = fields[sb["field"]]
        keys = fd.get("keys")
        src = dict(name=sb["name"], type=typ, field=sb["field"], interval=None, keys=keys, rank=None, sorted_keys=None)
        spec.sources[i].field = int(fd["id"])
        if typ == "terms":
            if keys is None:
                raise ValueError(f"aggregation {name!r}: terms source {sb['name']!r} needs a keyword field")
            raw = [k.encode("utf-8") for k in keys]
            if len(set(raw)) != len(raw):
                raise ValueError(f"aggregation {name!r}: the dictionary of {sb['field']!r} holds a key twice")
            order = sorted(range(len(raw)), key=lambda o: raw[o])  # (Rust orders String by its UTF-8 bytes)
            rank = np.zeros(len(raw), dtype=np.uint32)
            rank[np.asarray(order, dtype=np.int64)] = np.arange(len(raw), dtype=np.uint32)
            src["rank"], src["sorted_keys"] = rank, [keys[o] for o in order]
            spec.sources[i].kind = N.COMPOSITE_TERMS
            # (a dictionary registered in byte order needs no table: one dependent load less per value)
            presorted = order == list(range(len(raw)))
            spec.sources[i].ord_rank = None if presorted else rank.ctypes.data
        else:
            if keys is not None:
                raise ValueError(f"aggregation {name!r}: histogram source {sb['name']!r} needs a numeric field")
            src["interval"] = float(sb["interval"])
            spec.sources[i].kind, spec.sources[i].interval = N.COMPOSITE_HISTOGRAM, src["interval"]
        sources.append(src)
    children = agg_spec(body.get("aggs") or {}, fields)
    if children.top_hits_nodes or children.composite is not None:
        raise ValueError(f"aggregation {name!r}: top_hits or composite under a composite is not built on the device")
    for nd in children.nodes:
        if nd["parent"] >= 0:
            raise ValueError(f"aggregation {name!r}: only one level under a composite is built")
        if nd["type"] in VALUE_TYPES:
            raise ValueError(f"aggregation {name!r}: a {nd['type']} child of a composite is not built on the device")
    spec.n_children = len(children.nodes)
    for i in range(min(len(children.nodes), N.MAX_AGGS)):
        C.memmove(C.addressof(spec.children[i]), C.addressof(children.spec.nodes[i]), C.sizeof(N.AggNode))
    return dict(name=name, body=body, spec=spec, size=size, after=body.get("after"), sources=sources,
                children=children)


TERM_BUCKET_TYPES = ("significant_terms", "rare_terms")


def _byte_order_rank(name: str, field: str, keys: List[str]):
    """rank[ord] = the rank of ordinal ord's key in UTF-8 byte order (Rust orders String by its bytes), or None when
    the dictionary already is in that order (no table: one dependent load less per value)"""
    raw = [k.encode("utf-8") for k in keys]
    if len(set(raw)) != len(raw):
        raise ValueError(f"aggregation {name!r}: the dictionary of {field!r} holds a key twice")
    order = sorted(range(len(raw)), key=lambda o: raw[o])
    if order == list(range(len(raw))):
        return None
    rank = np.zeros(len(raw), dtype=np.uint32)
    rank[np.asarray(order, dtype=np.int64)] = np.arange(len(raw), dtype=np.uint32)
    return rank


def _term_bucket_node(name: str, body: dict, fields: Dict[str, dict], out: "N.TermBucketNode") -> dict:
    """one significant_terms / rare_terms body -> a node of AggPlan.term_buckets, `out` filled; ValueError for what
    the device does not build"""
    typ = body["type"]
    if body.get("sampling") is not None:
        raise ValueError(f"aggregation {name!r}: sampling is not built on the device")
    if body.get("size") is None:
        raise ValueError(f"aggregation {name!r}: {typ} without `size` (all buckets) is not built on the device")
    size = int(body["size"])
    if size <= 0 or size > N.MAX_TERM_BUCKET_SIZE:
        raise ValueError(f"aggregation {name!r}: {typ} size {size} is not built on the device "
                         f"(1 .. {N.MAX_TERM_BUCKET_SIZE})")
    if body["field"] not in fields or body["field"] == FILTERS:
        raise ValueError(f"aggregation {name!r}: field {body['field']!r} is not registered")
    fd = fields[body["field"]]
    keys = fd.get("keys")
    if keys is None:
        raise ValueError(f"aggregation {name!r}: {typ} needs a keyword field")
    rank = _byte_order_rank(name, body["field"], keys)
    out.field, out.size = int(fd["id"]), size
    out.ord_rank = None if rank is None else rank.ctypes.data
    out.background_filter = -1
    if typ == "significant_terms":
        out.kind = N.TERMS_SIGNIFICANT
        mdc = body.get("min_doc_count")
        out.doc_count_bound = 1 if mdc is None else int(mdc)
        if body.get("background_filter") is not None:
            if not callable(fields.get(FILTERS)):
                raise ValueError(f"aggregation {name!r}: a background_filter needs fields[{FILTERS!r}], the map from "
                                 "a filter to a registered filter id")
            out.background_filter = int(fields[FILTERS](body["background_filter"]))
    else:
        out.kind = N.TERMS_RARE
        mdc = body.get("max_doc_count")
        out.doc_count_bound = 1 if mdc is None else int(mdc)
    children = agg_spec(body.get("aggs") or {}, fields)
    if children.top_hits_nodes or children.composite is not None or children.term_buckets is not None:
        raise ValueError(f"aggregation {name!r}: top_hits, composite, significant_terms or rare_terms under a {typ} "
                         "is not built on the device")
    for nd in children.nodes:
        if nd["parent"] >= 0:
            raise ValueError(f"aggregation {name!r}: only one level under a {typ} is built")
        if nd["type"] in VALUE_TYPES:
            raise ValueError(f"aggregation {name!r}: a {nd['type']} child of a {typ} is not built on the device")
    out.n_children = len(children.nodes)
    for i in range(min(len(children.nodes), N.MAX_AGGS)):
        C.memmove(C.addressof(out.children[i]), C.addressof(children.spec.nodes[i]), C.sizeof(N.AggNode))
    return dict(name=name, type=typ, body=body, field=body["field"], size=size, keys=list(keys), rank=rank,
                children=children)


def _top_hits_node(name: str, body: dict, parent: int, fields: Dict[str, dict]) -> dict:
    """one top_hits body -> dict(name, parent, from, size, sort); ValueError for what the device does not build"""
    if body.get("aggs"):
        raise ValueError(f"aggregation {name!r}: a top_hits aggregation has no children")
    if body.get("size") is None:  # (TopHitsAggregation::size has no default: the reference refuses the request)
        raise ValueError(f"aggregation {name!r}: top_hits requires `size`")
    size, frm = int(body["size"]), int(body.get("from") or 0)
    if size == 0:
        raise ValueError(f"aggregation {name!r}: top_hits size 0 is not built on the device (nothing to select)")
    if frm < 0 or size < 0 or frm + size > N.MAX_TOP_HITS:
        raise ValueError(f"aggregation {name!r}: top_hits from + size > {N.MAX_TOP_HITS} is not built on the device")
    sort = []
    for part in body.get("sort") or []:
        field, order = (part.get("field"), part.get("order")) if isinstance(part, dict) else part
        if order is None:  # default_order_for_field (query/sort.rs:392-398)
            order = "desc" if field == "_score" else "asc"
        if order not in ("asc", "desc"):
            raise ValueError(f"aggregation {name!r}: unknown sort order {order!r}")
        if field != "_score":
            if field not in fields or field == FILTERS:
                raise ValueError(f"aggregation {name!r}: sort field {field!r} is not registered")
            if fields[field].get("sort_id") is None:
                what = "a keyword sort part" if fields[field].get("keys") is not None else "a field without a sort column"
                raise ValueError(f"aggregation {name!r}: {what} ({field!r}) is not built on the device")
            field = int(fields[field]["sort_id"])
        sort.append((field, order))
    if len(sort) > N.MAX_SORT_PARTS:
        raise ValueError(f"aggregation {name!r}: more than {N.MAX_SORT_PARTS} sort parts are not built on the device")
    return {"name": name, "parent": parent, "from": frm, "size": size, "sort": sort}


def agg_spec(aggs: Dict[str, dict], fields: Dict[str, dict], top_hits_max_entries: int = 0) -> AggPlan:
    """aggs: the request's `aggs` map; fields: field name -> {"id": agg field id, "keys": [dictionary strings]
    (keyword fields)}.  fields[FILTERS], when given, is a callable: the `filter` body of a filter aggregation ->
    the id of a registered filter that stands for it (the caller compiles and registers it, searchlite_amd.filters;
    in the spirit of compile_filter's `nested` callback); without it a filter aggregation raises ValueError.
    Roots in name order, each followed by its children in name order.  Raises ValueError for what the device does
    not build (other types, deeper nesting, sampling) — such a request stays on the CPU path — and for a
    date_histogram request the reference refuses (validate_date_histogram_config).
    A top_hits aggregation names its sort fields through `fields` too: fields[name]["sort_id"] is the id of the
    registered sort field (GpuIndex.add_sort_field); a field with "keys" and no "sort_id" is a keyword sort part,
    which the device does not build; more than N.MAX_TOP_HITS_NODES top_hits aggregations raise ValueError too.
    top_hits_max_entries: slg_top_hits_spec.max_entries, the bucket-run slots of one query that a top_hits child of a
    terms, histogram, range or date_histogram aggregation may fill (the sum of its parent's counts).  The batch holds
    8 bytes per slot and query: the default 0 is the library's 2^19 slots, 4 MB per query (4 GB for 1024 queries), so
    a caller who knows a bound on the matched docs (times the values per doc of the parent's column) passes it; a
    query that needs more gets status 1 and goes to the CPU path.
    A root composite aggregation becomes AggPlan.composite (one per request; terms sources need fields[f]["keys"],
    whose UTF-8 byte order gives the rank permutation); ValueError for a dictionary that holds a key twice, a composite
    anywhere but the root, a second one, sampling, pipeline, top_hits or value-node children, a third level, and a
    size of 0 or above N.MAX_COMPOSITE_SIZE."""
    nodes: List[dict] = []
    th_nodes: List[dict] = []
    composite: List[dict] = []
    term_buckets: List[tuple] = []  # (name, body) of the root significant_terms / rare_terms aggregations

    def add(name, body, parent):
        typ = body.get("type")
        if typ in TERM_BUCKET_TYPES:  # (beside the spec, as a composite: at the root only)
            if parent >= 0:
                raise ValueError(f"aggregation {name!r}: a {typ} below another aggregation is not built on the device")
            term_buckets.append((name, body))
            return
        if typ == "composite":  # (beside the spec, as top_hits: at the root only, one per request)
            if parent >= 0:
                raise ValueError(f"aggregation {name!r}: a composite below another aggregation is not built on the device")
            if composite:
                raise ValueError(f"aggregation {name!r}: a second composite is not built on the device")
            composite.append(_composite_plan(name, body, fields))
            return
        if typ == "top_hits":  # (beside the spec: a child only of a root bucket aggregation, which its parent checked)
            th_nodes.append(_top_hits_node(name, body, parent, fields))
            return
        if typ not in KINDS:
            raise ValueError(f"aggregation {name!r}: type {typ!r} is not built on the device")
        if body.get("sampling") is not None:
            raise ValueError(f"aggregation {name!r}: sampling is not built on the device")
        nd = dict(name=name, type=typ, body=body, parent=parent, keys=None)
        if typ == "filter":
            if not callable(fields.get(FILTERS)):
                raise ValueError(f"aggregation {name!r}: a filter aggregation needs fields[{FILTERS!r}], the map from "
                                 "its filter to a registered filter id")
            nd["filter"] = int(fields[FILTERS](body["filter"]))
        else:
            if body["field"] not in fields or body["field"] == FILTERS:
                raise ValueError(f"aggregation {name!r}: field {body['field']!r} is not registered")
            nd["keys"] = fields[body["field"]].get("keys")
        if typ == "date_histogram":
            nd["date"] = date_histogram_config(name, body)
        if typ == "date_range":
            nd["date_range"] = date_range_config(body)
        nodes.append(nd)
        me = len(nodes) - 1
        children = body.get("aggs") or {}
        if children and (parent >= 0 or typ not in BUCKET_TYPES):
            raise ValueError(f"aggregation {name!r}: only two levels under a bucket aggregation are built")
        for cname in sorted(children):
            add(cname, children[cname], me)

    for name in sorted(aggs):
        add(name, aggs[name], -1)
    spec = N.AggSpec()
    spec.n_nodes = len(nodes)
    for i, nd in enumerate(nodes[:N.MAX_AGGS]):  # (more are passed on as a count: the library refuses them)
        body, n = nd["body"], spec.nodes[i]
        n.kind, n.parent = KINDS[nd["type"]], nd["parent"]
        if nd["type"] == "filter":
            n.filter = nd["filter"]
            continue
        n.field = int(fields[body["field"]]["id"])
        missing = body.get("missing")
        if nd["type"] == "date_histogram":
            dh, missing = nd["date"], None
            n.calendar_unit, n.date_step, n.date_offset = dh["unit"], dh["step"], dh["offset"]
            if dh["missing"] is not None:
                n.has_missing, n.missing = 1, float(dh["missing"])
            if dh["hard"] is not None:
                n.has_hard_bounds, n.date_hard_min, n.date_hard_max = 1, dh["hard"][0], dh["hard"][1]
        if nd["type"] == "date_range":
            dr, missing = nd["date_range"], None
            if dr["missing"] is not None:
                n.has_missing, n.missing = 1, dr["missing"]
            n.n_ranges = len(dr["ranges"])
            for r, (_, lo, hi) in enumerate(dr["ranges"][:N.MAX_AGG_RANGES]):
                n.from_[r] = -math.inf if lo is None else lo
                n.to[r] = math.inf if hi is None else hi
        if nd["type"] == "terms" or (nd["type"] == "cardinality" and nd["keys"] is not None):
            if missing is not None:
                keys = list(nd["keys"] or [])
                n.has_missing = 1
                n.missing_ord = keys.index(str(missing)) if str(missing) in keys else len(keys)
        elif missing is not None:
            n.has_missing, n.missing = 1, float(missing)
        if nd["type"] in ("percentiles", "percentile_ranks"):
            xs = node_percents(body)
            n.n_ranges = len(xs)
            for r, x in enumerate(xs[:N.MAX_AGG_RANGES]):
                n.from_[r] = x
        if nd["type"] == "histogram":
            n.interval, n.offset = float(body["interval"]), float(body.get("offset") or 0.0)
            hb = body.get("hard_bounds")
            if hb is not None:
                n.has_hard_bounds, n.hard_min, n.hard_max = 1, float(hb["min"]), float(hb["max"])
        if nd["type"] == "range":
            ranges = body["ranges"]
            n.n_ranges = len(ranges)
            for r, rg in enumerate(ranges[:N.MAX_AGG_RANGES]):
                n.from_[r] = -math.inf if rg.get("from") is None else float(rg["from"])
                n.to[r] = math.inf if rg.get("to") is None else float(rg["to"])
    th_spec = None
    if len(th_nodes) > N.MAX_TOP_HITS_NODES:
        raise ValueError(f"more than {N.MAX_TOP_HITS_NODES} top_hits aggregations are not built on the device")
    if th_nodes:
        th_spec = N.TopHitsSpec()
        th_spec.n_nodes = len(th_nodes)
        th_spec.max_entries = int(top_hits_max_entries)
        for j, th in enumerate(th_nodes):
            t = th_spec.nodes[j]
            t.parent, t.from_, t.size = th["parent"], th["from"], th["size"]
            t.sort.n_parts = len(th["sort"])
            for i, (field, order) in enumerate(th["sort"]):
                t.sort.field[i] = N.SORT_SCORE if field == "_score" else field
                t.sort.order[i] = N.ORDER_ASC if order == "asc" else N.ORDER_DESC
    tb = None
    if len(term_buckets) > N.MAX_TERM_BUCKET_NODES:
        raise ValueError(f"more than {N.MAX_TERM_BUCKET_NODES} significant_terms / rare_terms aggregations are not built "
                         "on the device")
    if term_buckets:
        if composite or th_nodes:
            raise ValueError("significant_terms / rare_terms together with a composite or top_hits aggregation is not "
                             "built on the device")
        tb_spec = N.TermBucketSpec()
        tb_spec.n_nodes = len(term_buckets)
        tb = dict(spec=tb_spec, nodes=[_term_bucket_node(name, body, fields, tb_spec.nodes[i])
                                       for i, (name, body) in enumerate(term_buckets)])
    return AggPlan(spec, nodes, th_spec, th_nodes, composite[0] if composite else None, tb)


def _stats(cell) -> dict:
    count = int(cell["count"])
    s = float(cell["sum"])
    return {"type": "stats", "count": count, "min": float(cell["min"]), "max": float(cell["max"]), "sum": s,
            "avg": s / count if count > 0 else 0.0}


def _bucket_key_string(key) -> str:
    return key if isinstance(key, str) else json.dumps(key)


def f64_order_key(x: float) -> int:
    """the u64 whose integer order is f64::total_cmp (slg::agg_f64_key): -0.0 < 0.0, NaNs at the ends"""
    b = int(np.float64(x).view(np.uint64))
    return (~b) & 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def composite_slot_value(src_layout: dict, interval: float, slot: int) -> float:
    """the key of a histogram source's slot: -0.0, or float(id) * interval"""
    z = src_layout["zero_slot"]
    if z >= 0 and slot == z:
        return -0.0
    return float(src_layout["first_id"] + slot - (1 if z >= 0 and slot > z else 0)) * interval


def composite_lower_bound(layout: dict, plan: AggPlan, after) -> int:
    """The INCLUSIVE packed lower bound of "tuple > after" (finalize_composite, :3317-3337): layout =
    PreparedBatch.composite_layout().  Parts are walked in order; the first part that is not exactly a slot (a terms
    string absent from the dictionary, a histogram value that is not bitwise some slot's key) turns the strict
    comparison into "prefix equal and slot >= the first slot above it": that slot, zeros behind it.  When every part
    is a slot the bound is packed + 1.  A part above every slot carries into the prefix by itself (the bound is an
    integer, not a tuple); past the largest possible key the bound is 1 << key_bits (nothing follows).  An `after`
    the reference ignores (not an object, a missing name, a non-string terms part, a non-number histogram part) is 0."""
    cp = plan.composite
    if after is None or not isinstance(after, dict):
        return 0
    lays = layout["sources"]
    nothing = 1 << layout["key_bits"]
    max_key = sum((L["slots"] - 1) << L["shift"] for L in lays)
    packed = 0
    for src, L in zip(cp["sources"], lays):
        if src["name"] not in after:
            return 0
        v = after[src["name"]]
        if src["type"] == "terms":
            if not isinstance(v, str):
                return 0
            raw = v.encode("utf-8")
            keys = src["sorted_keys"]
            lo, hi = 0, len(keys)
            while lo < hi:  # the first slot whose key is >= v
                mid = (lo + hi) // 2
                if keys[mid].encode("utf-8") < raw:
                    lo = mid + 1
                else:
                    hi = mid
            exact = lo < len(keys) and keys[lo].encode("utf-8") == raw
        else:
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                return 0
            want = f64_order_key(float(v))
            n_real = L["slots"]  # (a column without a value has one slot, never emitted: any bound is right for it)
            lo, hi = 0, n_real
            while lo < hi:
                mid = (lo + hi) // 2
                if f64_order_key(composite_slot_value(L, src["interval"], mid)) < want:
                    lo = mid + 1
                else:
                    hi = mid
            exact = lo < n_real and f64_order_key(composite_slot_value(L, src["interval"], lo)) == want
        packed += lo << L["shift"]
        if not exact:
            return packed if packed <= max_key else nothing
    packed += 1
    return packed if packed <= max_key else nothing


def shape_composite(plan: AggPlan, layout: dict, page: dict, q: int) -> dict:
    """The response of query q's composite: {"type": "composite", "buckets": [{"key": {name: string | f64},
    "doc_count", "aggregations"}], "after_key"} — buckets ascending, after_key (the last bucket's key) only when
    there are more.  layout: PreparedBatch.composite_layout(); page: PreparedBatch.composite()."""
    cp = plan.composite
    lays = layout["sources"]
    kids = cp["children"]
    buckets = []
    for r in range(int(page["n_buckets"][q])):
        packed = int(page["keys"][q, r])
        key = {}
        for src, L in zip(cp["sources"], lays):
            slot = (packed >> L["shift"]) & ((1 << L["bits"]) - 1)
            key[src["name"]] = src["sorted_keys"][slot] if src["type"] == "terms" else \
                composite_slot_value(L, src["interval"], slot)
        b = {"key": key, "doc_count": int(page["counts"][q, r])}
        if kids.nodes:  # (shaped by the code that shapes any bucket's children: the children as roots, at row r)
            b["aggregations"] = shape(kids, layout["children"], page["children"], q, prow=r)
        buckets.append(b)
    out = {"type": "composite", "buckets": buckets}
    if int(page["has_more"][q]) and buckets:
        out["after_key"] = buckets[-1]["key"]
    return out


def shape_term_buckets(plan: AggPlan, layout: dict, fetched: dict, q: int) -> Dict[str, dict]:
    """The responses of query q's significant_terms / rare_terms aggregations by name: {"type": "significant_terms",
    "buckets": [{"key", "doc_count", "bg_count", "score", "aggregations"}], "doc_count", "bg_count"} in (score desc,
    count desc, key asc) order and {"type": "rare_terms", "buckets": [{"key", "doc_count", "aggregations"}]} in (count
    asc, key asc) order (finalize, :2515-2595).  layout: PreparedBatch.term_buckets_layout(); fetched:
    PreparedBatch.term_buckets()."""
    out = {}
    for nd, lay, got in zip(plan.term_buckets["nodes"], layout["nodes"], fetched["nodes"]):
        sig = nd["type"] == "significant_terms"
        kids = nd["children"]
        buckets = []
        for r in range(int(got["n_buckets"][q])):
            b = {"key": nd["keys"][int(got["ords"][q, r])], "doc_count": int(got["doc_counts"][q, r])}
            if sig:
                b["bg_count"], b["score"] = int(got["bg_counts"][q, r]), float(got["scores"][q, r])
            if kids.nodes:  # (the children as roots, at row r: as a composite's)
                b["aggregations"] = shape(kids, lay["children"], got["children"], q, prow=r)
            buckets.append(b)
        res = {"type": nd["type"], "buckets": buckets}
        if sig:
            res["doc_count"], res["bg_count"] = int(got["doc_count"][q]), int(got["bg_count"][q])
        out[nd["name"]] = res
    return out


def shape(plan: AggPlan, layout: List[dict], tables: List[np.ndarray], q: int, top_hits: Optional[dict] = None,
          matched=None, prow: int = 0, composite: Optional[tuple] = None,
          term_buckets: Optional[tuple] = None) -> Dict[str, dict]:
    """The response of query q: name -> AggregationResponse as a dict ({"type": ..., "buckets": [{"key",
    "doc_count", "aggregations"}]} / stats).  layout: PreparedBatch.agg_layout(); tables: PreparedBatch.aggs().
    top_hits: PreparedBatch.top_hits() of a plan with top_hits nodes, matched: PreparedBatch.matched_counts() (a
    root node's total): {"type": "top_hits", "total", "hits": [{"segment", "doc", "score"}]} at the root or in the
    bucket.  `fields` and `snippet` of a hit are doc-store work and are not part of it.  ValueError for a query
    whose bucket runs did not fit (status 1: the CPU path).  prow: the parent row the roots are read at (0; a
    composite's children are shaped as roots at their bucket's row).  composite: (PreparedBatch.composite_layout(),
    PreparedBatch.composite()) of a plan with a composite: its response goes under its name (shape_composite).
    term_buckets: (PreparedBatch.term_buckets_layout(), PreparedBatch.term_buckets()) of a plan with significant_terms
    or rare_terms aggregations: their responses go under their names (shape_term_buckets)."""
    if plan.top_hits_nodes and top_hits is not None and int(top_hits["status"][q]) != 0:
        raise ValueError(f"query {q}: the top_hits bucket runs did not fit max_entries (CPU path)")

    def hits_of(j: int, row: int, total: int) -> dict:
        arr = top_hits["nodes"][j]
        n = int(arr["count"][q, row])
        return {"type": "top_hits", "total": int(total),
                "hits": [{"segment": int(arr["seg"][q, row, i]), "doc": int(arr["doc"][q, row, i]),
                          "score": float(arr["score"][q, row, i])} for i in range(n)]}

    def top_hits_under(i: int, row: int, total: int) -> dict:
        if top_hits is None:
            return {}
        return {th["name"]: hits_of(j, row, total) for j, th in enumerate(plan.top_hits_nodes) if th["parent"] == i}

    def node(i: int, prow: int) -> dict:
        nd, body, tab = plan.nodes[i], plan.nodes[i]["body"], tables[i][q, prow]
        if nd["type"] == "stats":
            return _stats(tab[0])
        if nd["type"] == "value_count":  # :2685-2687
            return {"type": "value_count", "value": int(tab[0]["count"])}
        if nd["type"] == "cardinality":  # :2688-2692
            return {"type": "cardinality", "value": int(tab[0])}
        if nd["type"] == "percentiles":  # :3245-3251 (a BTreeMap: a repeated key keeps its last value)
            n = int(tab[0])
            return {"type": "percentiles",
                    "values": {rust_f64(p): percentile_of(n, int(tab[1 + 2 * j]), int(tab[2 + 2 * j]), p)
                               for j, p in enumerate(node_percents(body))}}
        if nd["type"] == "percentile_ranks":  # :547-553, :3253-3262
            n = int(tab[0])
            return {"type": "percentile_ranks",
                    "values": {rust_f64(t): (float(int(tab[1 + j])) / float(max(n, 1))) * 100.0 if n else 0.0
                               for j, t in enumerate(node_percents(body))}}
        children = [c for c in range(len(plan.nodes)) if plan.nodes[c]["parent"] == i]

        def bucket(key, row: Optional[int], count: int) -> dict:
            b = {"key": key, "doc_count": int(count)}
            if row is not None:
                kids = {plan.nodes[c]["name"]: node(c, row) for c in children}
                kids.update(top_hits_under(i, row, count))
                if kids:
                    b["aggregations"] = kids
            return b

        if nd["type"] == "filter":  # :2707-2726: the one bucket's children are the response's
            kids = {plan.nodes[c]["name"]: node(c, 0) for c in children}
            kids.update(top_hits_under(i, 0, int(tab[0])))
            return {"type": "filter", "doc_count": int(tab[0]), "aggregations": kids}
        if nd["type"] == "date_histogram":  # DateHistogramCollector::finish, :1364-1403
            dh = nd["date"]
            unit, step, offset = dh["unit"], dh["step"], dh["offset"]
            first = int(layout[i]["first_id"])
            found = {bucket_key(first + r, offset, unit, step): (r, int(tab[r])) for r in range(len(tab)) if int(tab[r]) > 0}
            bounds = dh["extended"] if dh["extended"] is not None else dh["hard"]
            if bounds is not None:
                start, end = (bucket_start(v, offset, unit, step) for v in bounds)
                if start > end:
                    start, end = end, start
                current = start
                while current is not None and current <= end:
                    found.setdefault(current, (None, 0))
                    current = add_interval(current, unit, step)
            mdc = body.get("min_doc_count")
            min_count = int(mdc) if mdc is not None else 0
            return {"type": "date_histogram",
                    "buckets": [bucket(key, r, c) for key, (r, c) in sorted(found.items()) if c >= min_count]}
        if nd["type"] == "date_range":  # the inner RangeCollector's buckets under the parsed bounds
            out = []
            for r, (key, lo, hi) in enumerate(nd["date_range"]["ranges"]):
                out.append(bucket(key if key is not None else {"from": lo, "to": hi}, r, int(tab[r])))
            return {"type": "date_range", "buckets": out, "keyed": bool(body.get("keyed", False))}
        if nd["type"] == "terms":
            keys = list(nd["keys"] or [])
            min_count = int(body.get("min_doc_count", 1) if body.get("min_doc_count") is not None else 1)
            rows = []
            for r in range(len(tab)):
                c = int(tab[r])
                if c == 0 or c < min_count:  # (a bucket exists once a doc was counted in it)
                    continue
                rows.append((keys[r] if r < len(keys) else body.get("missing"), r, c))
            rows.sort(key=lambda t: (-t[2], _bucket_key_string(t[0])))
            if body.get("size") is not None:
                rows = rows[:int(body["size"])]
            return {"type": "terms", "buckets": [bucket(k, r, c) for k, r, c in rows]}
        if nd["type"] == "histogram":
            interval, offset = float(body["interval"]), float(body.get("offset") or 0.0)
            bounds = body.get("extended_bounds") or body.get("hard_bounds")
            has_bounds = body.get("extended_bounds") is not None or body.get("hard_bounds") is not None
            mdc = body.get("min_doc_count")
            min_count = int(mdc) if mdc is not None else (0 if has_bounds else 1)
            first = int(layout[i]["first_id"])
            found = {first + r: (r, int(tab[r])) for r in range(len(tab)) if int(tab[r]) > 0}
            if bounds is not None:
                lo = math.floor((float(bounds["min"]) - offset) / interval)
                hi = math.floor((float(bounds["max"]) - offset) / interval)
                for bid in range(int(lo), int(hi) + 1):
                    found.setdefault(bid, (None, 0))
            return {"type": "histogram",
                    "buckets": [bucket(float(bid) * interval + offset, r, c)
                                for bid, (r, c) in sorted(found.items()) if c >= min_count]}
        ranges = body["ranges"]
        out = []
        for r, rg in enumerate(ranges):
            key = rg["key"] if rg.get("key") is not None else {"from": rg.get("from"), "to": rg.get("to")}
            out.append(bucket(key, r, int(tab[r])))
        return {"type": "range", "buckets": out, "keyed": bool(body.get("keyed", False))}

    out = {plan.nodes[i]["name"]: node(i, prow) for i in range(len(plan.nodes)) if plan.nodes[i]["parent"] < 0}
    if top_hits is not None and any(th["parent"] < 0 for th in plan.top_hits_nodes):
        if matched is None:
            raise ValueError("a root top_hits node needs `matched` (its total)")
        out.update(top_hits_under(-1, 0, int(matched[q])))
    if plan.composite is not None and composite is not None:
        out[plan.composite["name"]] = shape_composite(plan, composite[0], composite[1], q)
    if plan.term_buckets is not None and term_buckets is not None:
        out.update(shape_term_buckets(plan, term_buckets[0], term_buckets[1], q))
    return out
