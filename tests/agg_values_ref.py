"""A plain-Python restatement of the reference's cardinality, percentiles and percentile_ranks collectors and of
their finalisation (searchlite-core/src/query/aggs/mod.rs: QuantileState :472-553, CardinalityCollector
:1508-1556, finalize_response :2688-2702, compute_percentiles_from_state / _ranks_ :3245-3262), for the value-node
tests.  The bucket parents of a value child are tests/agg_ref.py's.

ONE DELIBERATE DEVIATION, the device's: the reference keeps every value only up to PERCENTILE_EXACT_LIMIT = 256
of them and answers from a t-digest beyond (:475-482, :539-544).  Here, as on the device, the exact formula of
the n <= 256 branch (:527-537, :552-553) is applied to ALL values whatever n is: equal to the reference where the
reference is exact, and the truth where it estimates.

  request   the reference's `aggs` map: name -> {"type", "field", ..., "aggs": {children}}
  columns   field name -> per_seg[s][doc] = list of the doc's values (strings for a keyword field)
  docs      the collected set: [(segment, doc)]
"""
import math
import struct

import numpy as np

from tests import agg_ref as R

VALUE_TYPES = ("cardinality", "percentiles", "percentile_ranks")
DEFAULT_PERCENTS = [1.0, 5.0, 25.0, 50.0, 75.0, 95.0, 99.0]  # default_percentiles_list (:3376-3378)
EXACT_LIMIT = 256  # PERCENTILE_EXACT_LIMIT: the reference is exact up to here


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def rust_f64(x):
    """format!("{x}") of an f64 (the response keys, :3248, :3257): shortest round-trip digits, no exponent, no
    trailing ".0"."""
    r = repr(float(x))
    if "e" in r:
        from decimal import Decimal
        r = format(Decimal(r), "f")
    return r[:-2] if r.endswith(".0") else r


def percents_of(body):
    if body["type"] == "percentiles":
        return [float(p) for p in (body["percents"] if body.get("percents") is not None else DEFAULT_PERCENTS)]
    return [float(v) for v in body["values"]]


def new_state(body):
    return {"type": body["type"], "set": set()} if body["type"] == "cardinality" else \
        {"type": body["type"], "values": []}


def collect(body, state, columns, seg, doc):
    values = columns[body["field"]][seg][doc]
    if body["type"] == "cardinality":  # :1508-1556: every value of the doc; `missing` for a doc without one
        if values and isinstance(values[0], str) or (not values and isinstance(body.get("missing"), str)):
            vals = list(values) or [body["missing"]]
            state["set"].update(vals)
        else:  # (hash of to_bits(): -0.0 and 0.0 are two values, :1549; distinct i64 are distinct f64 below 2^53)
            state["set"].update(f64_bits(v) for v in R.numeric_values(values, body.get("missing")))
        return
    state["values"].extend(R.numeric_values(values, body.get("missing")))  # QuantileState::push, exact branch


def rank_low_high(n, pct):
    """:529-532 -> (rank, low, high)"""
    rank = max((min(max(float(pct), 0.0), 100.0) / 100.0) * (float(n) - 1.0), 0.0)
    return rank, int(math.floor(rank)), int(math.ceil(rank))


def percentile(values, pct):
    """QuantileState::percentile, the exact branch (:523-537) over all values"""
    if not values:
        return 0.0
    vals = sorted(values)  # (partial_cmp: -0.0 and 0.0 compare equal; either order gives == results)
    rank, low, high = rank_low_high(len(vals), pct)
    if low == high:
        return vals[low]
    w = rank - float(low)
    return vals[low] * (1.0 - w) + vals[high] * w


def percentile_rank(values, target):
    """QuantileState::percentile_rank, the exact branch (:548-553)"""
    if not values:
        return 0.0
    return (float(sum(1 for v in values if v <= target)) / float(max(len(values), 1))) * 100.0


def respond_one(body, state):
    """finalize_response (:2688-2702); BTreeMap keys: a repeated key keeps its last value"""
    if body["type"] == "cardinality":
        return {"type": "cardinality", "value": len(state["set"])}
    f = percentile if body["type"] == "percentiles" else percentile_rank
    return {"type": body["type"], "values": {rust_f64(p): f(state["values"], p) for p in percents_of(body)}}


def strip(request):
    """the request without its value nodes (what tests/agg_ref.py collects); None when nothing is left"""
    out = {}
    for name, body in request.items():
        if body["type"] in VALUE_TYPES:
            continue
        b = dict(body)
        if body.get("aggs"):
            kids = strip(body["aggs"])
            if kids:
                b["aggs"] = kids
            else:
                del b["aggs"]
        out[name] = b
    return out


def run(request, columns, docs):
    """-> path -> state: path = (name,) for a value root, (parent name, bucket key, child name) for a value
    child, one state per parent bucket the doc was counted in (the bucket decision is agg_ref.collect's)."""
    states = {}
    for name, body in request.items():
        if body["type"] in VALUE_TYPES:
            st = states[(name,)] = new_state(body)
            for seg, doc in docs:
                collect(body, st, columns, seg, doc)
            continue
        kids = {c: b for c, b in (body.get("aggs") or {}).items() if b["type"] in VALUE_TYPES}
        if not kids:
            continue
        parent = {k: v for k, v in body.items() if k != "aggs"}
        for seg, doc in docs:
            one = R.new_state(parent)
            before = {k: b["doc_count"] for k, b in one["buckets"].items()}  # (range: every bucket pre-exists)
            R.collect(parent, one, columns, seg, doc)
            for key, b in one["buckets"].items():
                if b["doc_count"] == before.get(key, 0):
                    continue
                for cname, cbody in kids.items():
                    st = states.get((name, key, cname))
                    if st is None:
                        st = states[(name, key, cname)] = new_state(cbody)
                    collect(cbody, st, columns, seg, doc)
    return states


def value_rows(body):
    np_ = len(percents_of(body)) if body["type"] != "cardinality" else 0
    return {"cardinality": 1, "percentile_ranks": 1 + np_, "percentiles": 1 + 2 * np_}[body["type"]]


def ref_layout(nodes, columns, keys_of):
    """agg_ref.ref_layout with the value nodes' rows"""
    out = R.ref_layout(nodes, columns, keys_of)
    for lay, nd in zip(out, nodes):
        if nd["body"]["type"] in VALUE_TYPES:
            lay["rows"] = value_rows(nd["body"])
    return out


def cells(body, state):
    """one row of a value table (u64 cells): cardinality [count]; percentile_ranks [n, count(v <= t) per target];
    percentiles [n, bits(vals[low]), bits(vals[high]) per percent] (zeros when n == 0)"""
    if body["type"] == "cardinality":
        return [len(state["set"])]
    vals = state["values"]
    if body["type"] == "percentile_ranks":
        return [len(vals)] + [sum(1 for v in vals if v <= t) for t in percents_of(body)]
    out = [len(vals)]
    srt = sorted(vals)
    for p in percents_of(body):
        if not srt:
            out += [0, 0]
            continue
        _, low, high = rank_low_high(len(srt), p)
        out += [f64_bits(srt[low]), f64_bits(srt[high])]
    return out


def dense(nodes, layout, states, keys_of):
    """The states as the device's value tables: per node None (not a value node) or a uint64 array
    [parent_rows, rows].  nodes / layout as agg_ref.dense (layout from ref_layout above)."""
    out = []
    for i, nd in enumerate(nodes):
        body, lay = nd["body"], layout[i]
        if body["type"] not in VALUE_TYPES:
            out.append(None)
            continue
        tab = np.zeros((lay["parent_rows"], lay["rows"]), dtype=np.uint64)
        if nd["parent"] < 0:
            tab[0] = cells(body, states[(nd["name"],)])
        else:
            pn, pl = nodes[nd["parent"]], layout[nd["parent"]]
            for path, st in states.items():
                if len(path) != 3 or path[0] != pn["name"] or path[2] != nd["name"]:
                    continue
                pbody, key = pn["body"], path[1]
                if pbody["type"] == "terms":
                    keys = list(keys_of[pbody["field"]])
                    row = keys.index(key) if key in keys else len(keys)
                elif pbody["type"] == "histogram":
                    row = key - pl["first_id"]
                else:
                    row = key
                assert 0 <= row < pl["rows"]
                tab[row] = cells(body, st)
        out.append(tab)
    return out
