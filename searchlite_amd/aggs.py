"""Aggregations around the device tables (slg_batch_prepare_aggs): request -> slg_agg_spec, tables -> response.

The device returns raw dense tables per node (PreparedBatch.aggs()).  Everything after the tables is host
work and lives here, a restatement of the reference's finish / finalize steps (query/aggs/mod.rs):
terms buckets ordered by count descending, then key STRING ascending (terms_bucket_cmp, :2469-2478), `size`
and `min_doc_count` (default 1); histogram keys id * interval + offset, `min_doc_count` (default 0 with
bounds, else 1), zero buckets over extended_bounds (or hard_bounds), ascending; range buckets in request order
with their key string or {"from", "to"}; stats with avg = sum / count (0.0 when empty).

A request is the reference's `aggs` map: name -> {"type": "terms" | "histogram" | "range" | "stats",
"field": ..., ..., "aggs": {...children...}}.  Maps are walked in name order, as the reference's BTreeMaps.
"""
from __future__ import annotations

import json
import math
from typing import Dict, List, Optional

import numpy as np

from . import _native as N

KINDS = {"terms": N.AGG_TERMS, "histogram": N.AGG_HISTOGRAM, "range": N.AGG_RANGE, "stats": N.AGG_STATS}
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
        if children and (parent >= 0 or typ == "stats"):
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
        if nd["type"] == "terms":
            if missing is not None:
                keys = list(nd["keys"] or [])
                n.has_missing = 1
                n.missing_ord = keys.index(str(missing)) if str(missing) in keys else len(keys)
        elif missing is not None:
            n.has_missing, n.missing = 1, float(missing)
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
