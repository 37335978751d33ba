"""The reference's composite aggregation, restated for the tests (no line of it is copied).

query/aggs/mod.rs, CompositeCollector (:1689-1842) and finalize_composite (:3264-3368); the request types are
api/types.rs:694-718.

  sources     in request order: Terms {name, field} over a keyword fast field, Histogram {name, field, interval}
              over a numeric fast field; neither has `missing`, `offset` or bounds
  key part    terms: the dictionary string, ordered as Rust orders String (its UTF-8 bytes); histogram: the f64
              floor(v / interval) * interval, identity by BITS and order total_cmp (:1713-1727), so -0.0 and 0.0 are
              two buckets, -0.0 first
  collect     a doc with no value in any one source is skipped (:1793-1795); otherwise it is counted once in every
              DISTINCT tuple of the cross product of its values per source (:1800-1804), and the children of a bucket
              collect the doc once per tuple it was counted in.  A histogram source reads f64_values
              (index/fastfields.rs:754-770), which sees f64 columns only: over an i64 column every doc is skipped
  merge       segments merge by key without truncation (:2337-2363): one collector over all docs is the same
  finalize    buckets sorted by tuple (part by part, then length); only key > `after` kept, where an `after` that
              lacks a source's name or has a part of the wrong JSON type is IGNORED (:3274-3283, :3317-3337);
              has_more = len > size; truncate to size; after_key = the last kept bucket's key only when has_more

columns: field -> values[seg][doc] (lists; strings for a keyword field, numbers for a numeric one); f64_fields: the
numeric fields that are f64 columns.  Children are collected and rendered by tests/agg_date_ref.py, as under any
bucket.
"""
import numpy as np

from tests import agg_date_ref as D


def f64_order(x):
    """the integer whose order is f64::total_cmp"""
    b = int(np.float64(x).view(np.uint64))
    return (~b) & 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def hist_key(v, interval):
    """floor(v / interval) * interval, operation by operation in IEEE f64 (math.floor would lose -0.0)"""
    return float(np.floor(np.float64(v) / np.float64(interval)) * np.float64(interval))


def part_order(source, part):
    return part.encode("utf-8") if source["type"] == "terms" else f64_order(part)


def tuple_order(sources, key):
    return tuple(part_order(s, p) for s, p in zip(sources, key))


def doc_tuples(sources, columns, f64_fields, seg, doc):
    """the distinct tuples of one doc, identified by tuple_order (a float part by its bits) -> {order: key}"""
    per_source = []
    for s in sources:
        values = columns[s["field"]][seg][doc]
        if s["type"] == "histogram":
            values = [hist_key(v, s["interval"]) for v in values] if s["field"] in f64_fields else []
        if not values:
            return {}
        per_source.append(values)
    out = {(): ()}
    for s, values in zip(sources, per_source):
        out = {o + (part_order(s, v),): k + (v,) for o, k in out.items() for v in values}
    return out


def collect(sources, columns, f64_fields, docs):
    """-> {order: (key, [(seg, doc)] the docs counted in the bucket, each once)}"""
    buckets = {}
    for seg, doc in docs:
        for o, k in doc_tuples(sources, columns, f64_fields, seg, doc).items():
            buckets.setdefault(o, (k, []))[1].append((seg, doc))
    return buckets


def after_order(sources, after):
    """the comparable form of `after`, or None when the reference ignores it"""
    if not isinstance(after, dict):
        return None
    out = []
    for s in sources:
        if s["name"] not in after:
            return None
        v = after[s["name"]]
        if s["type"] == "terms":
            if not isinstance(v, str):
                return None
        elif isinstance(v, bool) or not isinstance(v, (int, float)):
            return None
        out.append(part_order(s, v if s["type"] == "terms" else float(v)))
    return tuple(out)


def finalize(sources, buckets, size, after=None):
    """-> ([(key, docs)] ascending, has_more)"""
    rows = sorted(buckets.items())
    bound = after_order(sources, after)
    if bound is not None:
        rows = [r for r in rows if r[0] > bound]
    has_more = len(rows) > size
    return [kd for _, kd in rows[:size]], has_more


def respond(body, columns, f64_fields, passes, docs):
    """the AggregationResponse of one composite body over the matched docs"""
    sources = body["sources"]
    rows, has_more = finalize(sources, collect(sources, columns, f64_fields, docs), body["size"], body.get("after"))
    kids = body.get("aggs") or {}
    out = []
    for key, bdocs in rows:
        b = {"key": {s["name"]: p for s, p in zip(sources, key)}, "doc_count": len(bdocs)}
        if kids:
            b["aggregations"] = D.respond(kids, D.run(kids, columns, passes, bdocs))
        out.append(b)
    resp = {"type": "composite", "buckets": out}
    if has_more and out:
        resp["after_key"] = out[-1]["key"]
    return resp


def same_key(a, b):
    """two bucket keys are the same: strings equal, floats equal by bits"""
    if a.keys() != b.keys():
        return False
    return all((x == y) if isinstance(x, str) else
               (not isinstance(y, str) and f64_order(x) == f64_order(y)) for x, y in ((a[n], b[n]) for n in a))
