"""A plain-Python restatement of the reference's terms, histogram, range and stats collectors and of the
shaping of their response (searchlite-core/src/query/aggs/mod.rs), for the aggregation tests.

Collectors keep hash maps, as the reference does; all segments feed ONE collector tree, which is the device's
deliberate deviation (the reference truncates terms buckets per segment before merging, :932-944).

  request   the reference's `aggs` map: name -> {"type", "field", ..., "aggs": {children}}
  columns   field name -> per_seg[s][doc] = list of the doc's values (strings for a keyword field, numbers
            for a numeric one; numbers reach the collectors as f64, index/fastfields.rs:772-800)
  docs      the collected set: [(segment, doc)]
"""
import json
import math

import numpy as np


def bucket_id(val, interval, offset):
    """HistogramCollector::bucket_key (:1162-1164): IEEE f64 subtraction, division, floor."""
    return int(math.floor((float(val) - float(offset)) / float(interval)))


def numeric_values(values, missing):
    """numeric_values (:597-610): the doc's values, or [missing] for a doc without one."""
    vals = [float(v) for v in values]
    if not vals and missing is not None:
        vals.append(float(missing))
    return vals


def new_state(body):
    if body["type"] == "stats":
        return {"type": "stats", "count": 0, "min": 0.0, "max": 0.0, "sum": 0.0}  # StatsState::default
    st = {"type": body["type"], "buckets": {}}
    if body["type"] == "range":  # (:1019-1030: every range has its bucket, and its children, from the start)
        for r in range(len(body["ranges"])):
            st["buckets"][r] = new_bucket(body)
    return st


def new_bucket(body):
    return {"doc_count": 0, "children": {n: new_state(b) for n, b in (body.get("aggs") or {}).items()}}


def collect(body, state, columns, seg, doc):
    values = columns[body["field"]][seg][doc]
    kind = body["type"]

    def into(key):
        b = state["buckets"].get(key)
        if b is None:
            b = state["buckets"][key] = new_bucket(body)
        b["doc_count"] += 1
        for name, child in (body.get("aggs") or {}).items():  # once per parent bucket (:905-908)
            collect(child, b["children"][name], columns, seg, doc)

    if kind == "terms":  # :894-930
        seen = []
        for v in values:
            if v not in seen:  # a doc counts once in every DISTINCT value
                seen.append(v)
                into(v)
        if not seen and body.get("missing") is not None:
            into(body["missing"])  # (the missing key may equal a real key: the same bucket)
        return
    vals = numeric_values(values, body.get("missing"))
    if kind == "stats":  # :1426-1441: every value of the doc
        for v in vals:
            if state["count"] == 0:
                state["min"] = state["max"] = v
            state["count"] += 1
            state["min"] = min(state["min"], v)
            state["max"] = max(state["max"], v)
            state["sum"] += v
        return
    if not vals:
        return
    if kind == "histogram":  # :1166-1204
        seen = set()
        hb = body.get("hard_bounds")
        for v in vals:
            if hb is not None and (v < hb["min"] or v > hb["max"]):
                continue
            bid = bucket_id(v, body["interval"], body.get("offset") or 0.0)
            if bid in seen:
                continue
            seen.add(bid)
            into(bid)
        return
    assert kind == "range"  # :1019-1030: `to` is inclusive
    for r, rg in enumerate(body["ranges"]):
        lo, hi = rg.get("from"), rg.get("to")
        if any((lo is None or v >= lo) and (hi is None or v <= hi) for v in vals):
            into(r)


def run(request, columns, docs):
    """-> name -> collector state after every doc of `docs`."""
    states = {name: new_state(body) for name, body in request.items()}
    for seg, doc in docs:
        for name, body in request.items():
            collect(body, states[name], columns, seg, doc)
    return states


def key_string(key):
    return key if isinstance(key, str) else json.dumps(key)


def respond_one(body, state):
    """finish + finalize of one aggregation -> its response."""
    if body["type"] == "stats":  # :2654-2664
        c = state["count"]
        return {"type": "stats", "count": c, "min": state["min"], "max": state["max"], "sum": state["sum"],
                "avg": state["sum"] / c if c > 0 else 0.0}

    def bucket(key, b):
        out = {"key": key, "doc_count": b["doc_count"]}
        if b["children"]:
            out["aggregations"] = {n: respond_one(body["aggs"][n], s) for n, s in sorted(b["children"].items())}
        return out

    buckets = state["buckets"]
    if body["type"] == "terms":  # :932-944 + terms_bucket_cmp :2469-2478
        mdc = body.get("min_doc_count")
        mdc = 1 if mdc is None else mdc
        rows = [(k, b) for k, b in buckets.items() if b["doc_count"] >= mdc]
        rows.sort(key=lambda kb: (-kb[1]["doc_count"], key_string(kb[0])))
        if body.get("size") is not None:
            rows = rows[:body["size"]]
        return {"type": "terms", "buckets": [bucket(k, b) for k, b in rows]}
    if body["type"] == "histogram":  # :1207-1245
        interval, offset = float(body["interval"]), float(body.get("offset") or 0.0)
        bounds = body.get("extended_bounds") or body.get("hard_bounds")
        mdc = body.get("min_doc_count")
        mdc = (0 if bounds is not None else 1) if mdc is None else mdc
        allb = dict(buckets)
        if bounds is not None:
            for bid in range(bucket_id(bounds["min"], interval, offset), bucket_id(bounds["max"], interval, offset) + 1):
                allb.setdefault(bid, {"doc_count": 0, "children": {}})  # (zero buckets carry no children)
        return {"type": "histogram", "buckets": [bucket(float(bid) * interval + offset, b)
                                                 for bid, b in sorted(allb.items()) if b["doc_count"] >= mdc]}
    out = []
    for r, rg in enumerate(body["ranges"]):  # :1032-1055
        key = rg["key"] if rg.get("key") is not None else {"from": rg.get("from"), "to": rg.get("to")}
        out.append(bucket(key, buckets[r]))
    return {"type": "range", "buckets": out, "keyed": bool(body.get("keyed", False))}


def respond(request, states):
    return {name: respond_one(body, states[name]) for name, body in sorted(request.items())}


STATS_DTYPE = np.dtype([("count", np.uint64), ("min", np.float64), ("max", np.float64), ("sum", np.float64)])


def histogram_id_range(body, all_values):
    """(first id, rows) of the dense table a histogram over a column holding `all_values` needs: the ids of the
    smallest and largest value that can be collected (the formula is monotone)."""
    vals = [float(v) for v in all_values]
    if body.get("missing") is not None:
        vals.append(float(body["missing"]))
    hb = body.get("hard_bounds")
    if vals and hb is not None:
        lo, hi = max(min(vals), hb["min"]), min(max(vals), hb["max"])
        vals = [lo, hi] if lo <= hi else []
    if not vals:
        return 0, 1
    off = body.get("offset") or 0.0
    a, b = bucket_id(min(vals), body["interval"], off), bucket_id(max(vals), body["interval"], off)
    return a, b - a + 1


def dense(nodes, layout, states, keys_of):
    """The collector states as the device's dense tables.  nodes: per node dict(name, body, parent) in the
    device's order (roots by name, each followed by its children by name); layout: per node dict(parent_rows,
    rows, first_id); keys_of: field -> the keyword dictionary.  -> per node an array [parent_rows, rows]
    (uint64 counts, or STATS_DTYPE).  A bucket outside a table is an error."""

    def row_of(body, lay, key):
        if body["type"] == "terms":
            keys = list(keys_of[body["field"]])
            r = keys.index(key) if key in keys else len(keys)
        elif body["type"] == "histogram":
            r = key - lay["first_id"]
        else:
            r = key
        assert 0 <= r < lay["rows"], (body["type"], key, lay)
        return r

    out = []
    for i, nd in enumerate(nodes):
        lay, body = layout[i], nd["body"]
        tab = np.zeros((lay["parent_rows"], lay["rows"]), dtype=STATS_DTYPE if body["type"] == "stats" else np.uint64)
        if nd["parent"] < 0:
            per_parent = {0: states[nd["name"]]}
        else:
            pn, pl = nodes[nd["parent"]], layout[nd["parent"]]
            per_parent = {row_of(pn["body"], pl, k): b["children"][nd["name"]]
                          for k, b in states[pn["name"]]["buckets"].items()}
        for prow, st in per_parent.items():
            if body["type"] == "stats":
                tab[prow, 0] = (st["count"], st["min"], st["max"], st["sum"])
            else:
                for k, b in st["buckets"].items():
                    tab[prow, row_of(body, lay, k)] += b["doc_count"]
        out.append(tab)
    return out


def ref_layout(nodes, columns, keys_of):
    """The layout the device must report for `nodes` over `columns`: per node dict(parent_rows, rows, first_id)."""
    out = []
    for nd in nodes:
        body = nd["body"]
        first, rows = 0, 1
        if body["type"] == "terms":
            keys = list(keys_of[body["field"]])
            rows = len(keys) + (1 if body.get("missing") is not None and body["missing"] not in keys else 0)
        elif body["type"] == "histogram":
            first, rows = histogram_id_range(body, [v for seg in columns[body["field"]] for d in seg for v in d])
        elif body["type"] == "range":
            rows = len(body["ranges"])
        out.append(dict(parent_rows=1 if nd["parent"] < 0 else out[nd["parent"]]["rows"], rows=rows, first_id=first))
    return out
