"""A plain-Python restatement of the reference's date_histogram, date_range, filter and value_count collectors and
of their finish / finalize steps (searchlite-core/src/query/aggs/mod.rs: DateHistogramCollector :1263-1404,
bucket_start / add_interval / truncate_calendar / add_calendar :3391-3465, parse_date / parse_interval_seconds
:3467-3498, DateRangeCollector :1063-1122, FilterCollector :1640-1687, ValueCountCollector :1448-1476,
finalize_response :2640-2726), for the date aggregation tests.  One collector tree over all segments, hash maps,
as tests/agg_ref.py; the older kinds (terms, histogram, range, stats: tests/agg_ref.py; cardinality,
percentile_ranks, percentiles: tests/agg_values_ref.py) are reached through those helpers, so that a tree may mix
them with the new kinds in either role.

Calendar arithmetic goes through `datetime` (proleptic Gregorian, years 1 .. 9999), NOT through the integer
days-to-civil algorithm the library uses.

  request   the reference's `aggs` map; a filter aggregation's `filter` is {"name": <key of `passes`>}
  columns   field name -> per_seg[s][doc] = list of the doc's values
  passes    filter name -> per_seg[s][doc] = bool (the doc passes)
  docs      the collected set: [(segment, doc)]
"""
import math
import re
from datetime import date, datetime, timedelta

import numpy as np

from tests import agg_ref as R
from tests import agg_values_ref as V

EPOCH = datetime(1970, 1, 1)
MS = timedelta(milliseconds=1)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
UNITS = {"day": "day", "1d": "day", "week": "week", "1w": "week", "month": "month", "1m": "month",
         "quarter": "quarter", "1q": "quarter", "year": "year", "1y": "year"}
OLD_BUCKETS = ("terms", "histogram", "range")
BUCKETS = OLD_BUCKETS + ("date_histogram", "date_range", "filter")


# the instants the calendar tests draw from (and +-1 ms around each): the epoch and the ms before it, a Monday, a
# Sunday | Monday boundary, the 1900 non-leap and 2000 / 2024 leap Februaries, year, quarter and month ends, and the
# two ends of the supported range
MIN_MS, MAX_MS = -62_135_596_800_000, 253_402_300_799_999  # 0001-01-01T00:00:00Z, 9999-12-31T23:59:59.999Z
EDGE_DATES = ["1970-01-01T00:00:00.000", "1969-12-31T23:59:59.999", "1969-12-29T00:00:00.000", "1970-01-04T00:00:00.000",
              "1970-01-05T00:00:00.000", "1900-02-28T00:00:00.000", "1900-03-01T00:00:00.000", "2000-02-29T00:00:00.000",
              "2023-12-31T23:59:59.999", "2024-01-01T00:00:00.000", "2024-02-29T00:00:00.000", "2024-03-31T00:00:00.000",
              "2024-04-01T00:00:00.000", "0001-01-01T00:00:00.000", "9999-12-31T23:59:59.999"]


def edge_instants():
    """-> sorted distinct ms: every EDGE_DATES instant and its two neighbours, within the supported range"""
    out = set()
    for text in EDGE_DATES:
        t = (datetime.strptime(text, "%Y-%m-%dT%H:%M:%S.%f") - EPOCH) // MS
        out.update(v for v in (t - 1, t, t + 1) if MIN_MS <= v <= MAX_MS)
    return sorted(out)


# ---- parsing -----------------------------------------------------------------------------------------------
def as_i64(x):
    """`x as i64`: toward zero, saturating, NaN -> 0"""
    if math.isnan(x):
        return 0
    if math.isinf(x):
        return I64_MAX if x > 0 else I64_MIN
    return min(max(math.trunc(x), I64_MIN), I64_MAX)


def parse_f64(s):
    try:
        return float(s) if isinstance(s, str) and s == s.strip() and "_" not in s and s else None
    except ValueError:
        return None


def parse_interval_seconds(spec):
    mt = re.match(r"[0-9.]+", spec)
    if not mt:
        return None
    value = parse_f64(mt.group(0))
    mult = {"": 1.0, "s": 1.0, "ms": 0.001, "m": 60.0, "h": 3600.0, "d": 86400.0, "w": 604800.0}.get(spec[mt.end():])
    return None if value is None or mult is None else value * mult


def parse_date(value):
    """RFC 3339 -> ms as f64, else a plain number"""
    mt = re.fullmatch(r"(\d{4}-\d\d-\d\d)[Tt ](\d\d:\d\d:\d\d)(\.\d+)?([Zz]|[+-]\d\d:\d\d)", value)
    if mt:
        try:
            dt = datetime.strptime(mt.group(1) + " " + mt.group(2), "%Y-%m-%d %H:%M:%S")
        except ValueError:
            dt = None
        if dt is not None:
            ms = (dt - EPOCH) // MS + int(((mt.group(3) or ".0")[1:] + "00")[:3])
            tz = mt.group(4)
            if tz not in "Zz":
                ms -= (1 if tz[0] == "+" else -1) * (int(tz[1:3]) * 60 + int(tz[4:6])) * 60000
            return float(ms)
    return parse_f64(value)


_CONFIGS = {}


def config(body):
    """DateHistogramCollector::new: -> dict(unit (None: fixed), step, offset, extended, hard, missing), i64 ms
    (kept per body object: the collectors ask once per doc)"""
    hit = _CONFIGS.get(id(body))
    if hit is None or hit[0] is not body:
        hit = _CONFIGS[id(body)] = (body, _config(body))
    return hit[1]


def _config(body):
    unit = UNITS.get((body.get("calendar_interval") or "").lower()) if body.get("calendar_interval") else None
    step = 0
    if unit is None:
        secs = parse_interval_seconds(body["fixed_interval"]) if body.get("fixed_interval") else None
        step = as_i64((86400.0 if secs is None else secs) * 1000.0)
    off = parse_interval_seconds(body["offset"]) if body.get("offset") else None
    cfg = dict(unit=unit, step=step, offset=0 if off is None else as_i64(off * 1000.0))
    for name, key in (("extended", "extended_bounds"), ("hard", "hard_bounds")):
        b, cfg[name] = body.get(key), None
        if b is not None:
            lo, hi = parse_date(b["min"]), parse_date(b["max"])
            if lo is not None and hi is not None:
                cfg[name] = (as_i64(lo), as_i64(hi))
    m = body.get("missing")
    m = float(m) if isinstance(m, (int, float)) else parse_date(m) if isinstance(m, str) else None
    cfg["missing"] = None if m is None else as_i64(m)
    cfg.update(body.get("_override") or {})  # (tests: an offset the request's strings cannot say, e.g. -3 ms)
    return cfg


# ---- calendar, through datetime ---------------------------------------------------------------------------------
def day_of(t):
    """the UTC date that holds instant t (floor: -1 ms is 1969-12-31)"""
    return (EPOCH + t * MS).date()


def ms_of(d):
    return (datetime(d.year, d.month, d.day) - EPOCH) // MS


def truncate_calendar(t, unit):
    d = day_of(t)
    if unit == "week":
        d = d - timedelta(days=d.weekday())
    elif unit == "month":
        d = d.replace(day=1)
    elif unit == "quarter":
        d = d.replace(month=(d.month - 1) // 3 * 3 + 1, day=1)
    elif unit == "year":
        d = d.replace(month=1, day=1)
    return ms_of(d)


def bucket_start(value, cfg):
    if cfg["unit"] is None:
        bucket = as_i64(float(math.ceil(float(value - cfg["offset"]) / float(cfg["step"]))))
        return min(max(bucket * cfg["step"], I64_MIN), I64_MAX) + cfg["offset"]
    return truncate_calendar(value - cfg["offset"], cfg["unit"]) + cfg["offset"]


def add_interval(current, cfg):
    unit = cfg["unit"]
    if unit is None:
        return current + cfg["step"] if current + cfg["step"] <= I64_MAX else None
    d = day_of(current)
    try:
        if unit == "day":
            d = d + timedelta(days=1)
        elif unit == "week":
            d = d + timedelta(days=7)
        elif unit == "month":
            y, m = (d.year + 1, 1) if d.month == 12 else (d.year, d.month + 1)
            d = d.replace(year=y).replace(month=m).replace(day=1)
        elif unit == "quarter":
            y, m = (d.year + 1, d.month - 9) if d.month + 3 > 12 else (d.year, d.month + 3)
            d = d.replace(year=y).replace(month=m).replace(day=1)
        else:
            d = d.replace(year=d.year + 1).replace(month=1).replace(day=1)
    except (ValueError, OverflowError):
        return None
    return ms_of(d)


def dense_id(value, cfg):
    """the device's row id of the bucket that holds `value` (include/searchlite_gpu.h), through datetime"""
    t = value - cfg["offset"]
    if cfg["unit"] is None:
        return int(math.ceil(float(t) / float(cfg["step"])))
    d = day_of(t)
    days = (d - date(1970, 1, 1)).days
    if cfg["unit"] == "day":
        return days
    if cfg["unit"] == "week":
        return ((d - timedelta(days=d.weekday())) - date(1969, 12, 29)).days // 7
    month = (d.year - 1970) * 12 + d.month - 1
    return {"month": month, "quarter": month // 3, "year": d.year - 1970}[cfg["unit"]]


def date_values(body, cfg, values):
    """numeric_values with `missing` (as f64), then `as i64` of each (:1320-1328)"""
    vals = [float(v) for v in values]
    if not vals and cfg["missing"] is not None:
        vals.append(float(cfg["missing"]))
    return [as_i64(v) for v in vals]


def date_range_config(body):
    as_str = lambda v: v if isinstance(v, str) else repr(v)
    ranges = [(rg.get("key"), None if rg.get("from") is None else parse_date(as_str(rg["from"])),
               None if rg.get("to") is None else parse_date(as_str(rg["to"]))) for rg in body["ranges"]]
    m = body.get("missing")
    m = parse_date(m) if isinstance(m, str) else float(m) if isinstance(m, (int, float)) else None
    return ranges, m


# ---- collectors ----------------------------------------------------------------------------------------------------
def childless(body):
    return {k: v for k, v in body.items() if k != "aggs"}


def new_state(body):
    t = body["type"]
    if t == "value_count":  # (the count of the stats state: the device keeps a whole stats cell for it)
        return R.new_state({"type": "stats"})
    if t in V.VALUE_TYPES:
        return V.new_state(body)
    if t == "stats":
        return R.new_state(body)
    st = {"type": t, "buckets": {}}
    if t in ("range", "date_range"):
        for r in range(len(body["ranges"])):
            st["buckets"][r] = new_bucket(body)
    if t == "filter":
        st["buckets"][0] = new_bucket(body)
    return st


def new_bucket(body):
    return {"doc_count": 0, "children": {n: new_state(b) for n, b in (body.get("aggs") or {}).items()}}


def buckets_of(body, columns, passes, seg, doc):
    """the keys of the buckets of `body` that one doc is counted in -> [(key, dense id or None)]"""
    t = body["type"]
    if t == "filter":
        return [(0, None)] if passes[body["filter"]["name"]][seg][doc] else []
    if t in OLD_BUCKETS:  # the bucket decision is agg_ref.collect's
        one = R.new_state(childless(body))
        before = {k: b["doc_count"] for k, b in one["buckets"].items()}
        R.collect(childless(body), one, columns, seg, doc)
        return [(k, None) for k, b in one["buckets"].items() if b["doc_count"] != before.get(k, 0)]
    values = columns[body["field"]][seg][doc]
    if t == "date_range":
        ranges, missing = date_range_config(body)
        vals = R.numeric_values(values, missing)
        return [(r, None) for r, (_, lo, hi) in enumerate(ranges)
                if any((lo is None or v >= lo) and (hi is None or v <= hi) for v in vals)]
    assert t == "date_histogram"
    cfg = config(body)
    out, seen = [], set()
    for val in date_values(body, cfg, values):  # :1333-1361
        if cfg["hard"] is not None and (val < cfg["hard"][0] or val > cfg["hard"][1]):
            continue
        key = bucket_start(val, cfg)
        if key in seen:
            continue
        seen.add(key)
        out.append((key, dense_id(val, cfg)))
    return out


def collect(body, state, columns, passes, seg, doc):
    t = body["type"]
    if t == "stats":
        return R.collect(body, state, columns, seg, doc)
    if t in V.VALUE_TYPES:
        return V.collect(body, state, columns, seg, doc)
    if t == "value_count":
        m = body.get("missing")
        m = float(m) if isinstance(m, (int, float)) else parse_f64(m) if isinstance(m, str) else None
        return R.collect({"type": "stats", "field": body["field"], "missing": m}, state, columns, seg, doc)
    for key, did in buckets_of(body, columns, passes, seg, doc):
        b = state["buckets"].get(key)
        if b is None:
            b = state["buckets"][key] = new_bucket(body)
        if did is not None:
            assert b.setdefault("id", did) == did, "the dense id is a function of the key"
        b["doc_count"] += 1
        for name, child in (body.get("aggs") or {}).items():
            collect(child, b["children"][name], columns, passes, seg, doc)


def run(request, columns, passes, docs):
    """-> name -> collector state after every doc of `docs`"""
    states = {name: new_state(body) for name, body in request.items()}
    for seg, doc in docs:
        for name, body in request.items():
            collect(body, states[name], columns, passes, seg, doc)
    return states


# ---- finish / finalize ------------------------------------------------------------------------------------------
def respond_one(body, state):
    t = body["type"]
    if t == "stats":
        return R.respond_one(body, state)
    if t in V.VALUE_TYPES:
        return V.respond_one(body, state)
    if t == "value_count":
        return {"type": "value_count", "value": state["count"]}

    def kids(b):
        return {n: respond_one(body["aggs"][n], s) for n, s in sorted(b["children"].items())}

    def bucket(key, b):
        out = {"key": key, "doc_count": b["doc_count"]}
        if b["children"]:
            out["aggregations"] = kids(b)
        return out

    buckets = state["buckets"]
    if t == "filter":
        return {"type": "filter", "doc_count": buckets[0]["doc_count"], "aggregations": kids(buckets[0])}
    if t == "date_histogram":  # finish, :1364-1403
        cfg = config(body)
        allb = dict(buckets)
        bounds = cfg["extended"] if cfg["extended"] is not None else cfg["hard"]
        if bounds is not None:
            start, end = bucket_start(bounds[0], cfg), bucket_start(bounds[1], cfg)
            if start > end:
                start, end = end, start
            current = start
            while current is not None and current <= end:
                allb.setdefault(current, {"doc_count": 0, "children": {}})
                current = add_interval(current, cfg)
        mdc = body.get("min_doc_count") or 0
        return {"type": "date_histogram", "buckets": [bucket(k, b) for k, b in sorted(allb.items()) if b["doc_count"] >= mdc]}
    if t == "date_range":
        ranges, _ = date_range_config(body)
        return {"type": "date_range", "keyed": bool(body.get("keyed", False)),
                "buckets": [bucket(key if key is not None else {"from": lo, "to": hi}, buckets[r])
                            for r, (key, lo, hi) in enumerate(ranges)]}
    if t == "terms":
        mdc = 1 if body.get("min_doc_count") is None else body["min_doc_count"]
        rows = [(k, b) for k, b in buckets.items() if b["doc_count"] >= mdc]
        rows.sort(key=lambda kb: (-kb[1]["doc_count"], R.key_string(kb[0])))
        if body.get("size") is not None:
            rows = rows[:body["size"]]
        return {"type": "terms", "buckets": [bucket(k, b) for k, b in rows]}
    if t == "histogram":
        interval, offset = float(body["interval"]), float(body.get("offset") or 0.0)
        bounds = body.get("extended_bounds") or body.get("hard_bounds")
        mdc = body.get("min_doc_count")
        mdc = (0 if bounds is not None else 1) if mdc is None else mdc
        allb = dict(buckets)
        if bounds is not None:
            for bid in range(R.bucket_id(bounds["min"], interval, offset), R.bucket_id(bounds["max"], interval, offset) + 1):
                allb.setdefault(bid, {"doc_count": 0, "children": {}})
        return {"type": "histogram", "buckets": [bucket(float(bid) * interval + offset, b)
                                                 for bid, b in sorted(allb.items()) if b["doc_count"] >= mdc]}
    out = []
    for r, rg in enumerate(body["ranges"]):
        key = rg["key"] if rg.get("key") is not None else {"from": rg.get("from"), "to": rg.get("to")}
        out.append(bucket(key, buckets[r]))
    return {"type": "range", "buckets": out, "keyed": bool(body.get("keyed", False))}


def respond(request, states):
    return {name: respond_one(body, states[name]) for name, body in sorted(request.items())}


# ---- the device's dense tables ----------------------------------------------------------------------------------
def date_id_range(body, all_values):
    """(first id, rows) of a date_histogram's dense table over a column holding `all_values`"""
    cfg = config(body)
    vals = [as_i64(float(v)) for v in all_values]
    if cfg["missing"] is not None:
        vals.append(cfg["missing"])
    if vals and cfg["hard"] is not None:
        lo, hi = max(min(vals), cfg["hard"][0]), min(max(vals), cfg["hard"][1])
        vals = [lo, hi] if lo <= hi else []
    if not vals:
        return 0, 1
    a, b = dense_id(min(vals), cfg), dense_id(max(vals), cfg)
    return a, b - a + 1


def ref_layout(nodes, columns, keys_of):
    """per node dict(parent_rows, rows, first_id), what the device must report"""
    out = []
    for nd in nodes:
        body = nd["body"]
        t, first, rows = body["type"], 0, 1
        if t == "date_histogram":
            first, rows = date_id_range(body, [v for seg in columns[body["field"]] for d in seg for v in d])
        elif t in ("date_range", "range"):
            rows = len(body["ranges"])
        elif t in V.VALUE_TYPES:
            rows = V.value_rows(body)
        elif t in ("terms", "histogram"):
            one = R.ref_layout([dict(body=body, parent=-1)], columns, keys_of)[0]
            first, rows = one["first_id"], one["rows"]
        out.append(dict(parent_rows=1 if nd["parent"] < 0 else out[nd["parent"]]["rows"], rows=rows, first_id=first))
    return out


def row_of(body, lay, key, b, keys_of):
    t = body["type"]
    if t == "terms":
        keys = list(keys_of[body["field"]])
        r = keys.index(key) if key in keys else len(keys)
    elif t == "histogram":
        r = key - lay["first_id"]
    elif t == "date_histogram":
        r = b["id"] - lay["first_id"]
    else:
        r = key  # range, date_range: the range's index; filter: 0
    assert 0 <= r < lay["rows"], (t, key, lay)
    return r


def dense(nodes, layout, states, keys_of):
    """The collector states as the device's tables: per node an array [parent_rows, rows] of uint64 counts (bucket
    kinds), agg_ref.STATS_DTYPE (stats, value_count) or uint64 value cells (cardinality, percentile_ranks,
    percentiles).  nodes: per node dict(name, body, parent) in the device's order."""
    out = []
    for i, nd in enumerate(nodes):
        lay, body = layout[i], nd["body"]
        t = body["type"]
        is_stats = t in ("stats", "value_count")
        tab = np.zeros((lay["parent_rows"], lay["rows"]), dtype=R.STATS_DTYPE if is_stats else np.uint64)
        if nd["parent"] < 0:
            per_parent = {0: states[nd["name"]]}
        else:
            pn, pl = nodes[nd["parent"]], layout[nd["parent"]]
            per_parent = {row_of(pn["body"], pl, k, b, keys_of): b["children"][nd["name"]]
                          for k, b in states[pn["name"]]["buckets"].items()}
        for prow, st in per_parent.items():
            if is_stats:
                tab[prow, 0] = (st["count"], st["min"], st["max"], st["sum"])
            elif t in V.VALUE_TYPES:
                tab[prow] = V.cells(body, st)
            else:
                for k, b in st["buckets"].items():
                    tab[prow, row_of(body, lay, k, b, keys_of)] += b["doc_count"]
        out.append(tab)
    return out
