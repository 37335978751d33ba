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

A request is the reference's `aggs` map: name -> {"type": "terms" | "histogram" | "range" | "stats" | "cardinality"
| "percentiles" | "percentile_ranks", "field": ..., ..., "aggs": {...children...}}.  Maps are walked in name order, as the reference's BTreeMaps.
"""
from __future__ import annotations

import json
import math
from typing import Dict, List, Optional

import numpy as np

from . import _native as N

KINDS = {"terms": N.AGG_TERMS, "histogram": N.AGG_HISTOGRAM, "range": N.AGG_RANGE, "stats": N.AGG_STATS,
         "cardinality": N.AGG_CARDINALITY, "percentiles": N.AGG_PERCENTILES, "percentile_ranks": N.AGG_PERCENTILE_RANKS}
BUCKET_TYPES = ("terms", "histogram", "range")
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
STATS_DTYPE = np.dtype([("count", np.uint64), ("min", np.float64), ("max", np.float64), ("sum", np.float64)])


class AggPlan:
    """A request's aggregations as the device takes them: .spec (N.AggSpec) and, per node in spec order,
    .nodes[i] = dict(name, type, body, parent, keys) for shape()."""

    def __init__(self, spec: "N.AggSpec", nodes: List[dict]):
        self.spec = spec
        self.nodes = nodes


def agg_spec(aggs: Dict[str, dict], fields: Dict[str, dict]) -> AggPlan:
    """aggs: the request's `aggs` map; fields: field name -> {"id": agg field id, "keys": [dictionary strings]
    (keyword fields)}.  Roots in name order, each followed by its children in name order.  Raises ValueError
    for what the device does not build (other types, deeper nesting, sampling): such a request stays on the
    CPU path."""
    nodes: List[dict] = []

    def add(name, body, parent):
        typ = body.get("type")
        if typ not in KINDS:
            raise ValueError(f"aggregation {name!r}: type {typ!r} is not built on the device")
        if body.get("sampling") is not None:
            raise ValueError(f"aggregation {name!r}: sampling is not built on the device")
        if body["field"] not in fields:
            raise ValueError(f"aggregation {name!r}: field {body['field']!r} is not registered")
        nodes.append(dict(name=name, type=typ, body=body, parent=parent, keys=fields[body["field"]].get("keys")))
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
        n.kind, n.field, n.parent = KINDS[nd["type"]], int(fields[body["field"]]["id"]), nd["parent"]
        missing = body.get("missing")
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
    return AggPlan(spec, nodes)


def _stats(cell) -> dict:
    count = int(cell["count"])
    s = float(cell["sum"])
    return {"type": "stats", "count": count, "min": float(cell["min"]), "max": float(cell["max"]), "sum": s,
            "avg": s / count if count > 0 else 0.0}


def _bucket_key_string(key) -> str:
    return key if isinstance(key, str) else json.dumps(key)


def shape(plan: AggPlan, layout: List[dict], tables: List[np.ndarray], q: int) -> Dict[str, dict]:
    """The response of query q: name -> AggregationResponse as a dict ({"type": ..., "buckets": [{"key",
    "doc_count", "aggregations"}]} / stats).  layout: PreparedBatch.agg_layout(); tables: PreparedBatch.aggs()."""

    def node(i: int, prow: int) -> dict:
        nd, body, tab = plan.nodes[i], plan.nodes[i]["body"], tables[i][q, prow]
        if nd["type"] == "stats":
            return _stats(tab[0])
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
            if row is not None and children:
                b["aggregations"] = {plan.nodes[c]["name"]: node(c, row) for c in children}
            return b

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

    return {plan.nodes[i]["name"]: node(i, 0) for i in range(len(plan.nodes)) if plan.nodes[i]["parent"] < 0}
