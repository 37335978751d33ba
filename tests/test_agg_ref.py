"""tests/agg_ref.py (the reference's collectors restated) pinned by hand-computed answers, and
searchlite_amd.aggs.shape (the host shaping of the device tables) checked against it.  No device."""
import numpy as np

from tests import agg_ref as R


def one_seg(**cols):
    """columns of one segment: name -> [values of doc 0, values of doc 1, ...]"""
    return {name: [docs] for name, docs in cols.items()}


def all_docs(columns):
    n = len(next(iter(columns.values()))[0])
    return [(0, d) for d in range(n)]


def both(request, columns, keys_of=None, docs=None):
    """-> (agg_ref's response, aggs.shape's response over agg_ref's dense tables) of one query"""
    from searchlite_amd import aggs as A
    keys_of = keys_of or {}
    docs = all_docs(columns) if docs is None else docs
    states = R.run(request, columns, docs)
    want = R.respond(request, states)
    fields = {name: {"id": i, "keys": keys_of.get(name)} for i, name in enumerate(sorted(columns))}
    plan = A.agg_spec(request, fields)
    layout = R.ref_layout(plan.nodes, columns, keys_of)
    tables = [t[None] for t in R.dense(plan.nodes, layout, states, keys_of)]
    return want, A.shape(plan, layout, tables, 0)


def counts(resp):
    return [(b["key"], b["doc_count"]) for b in resp["buckets"]]


def test_same_keyword_twice_counts_once():
    cols = one_seg(tag=[["a", "a", "b"], ["a"], []])
    want, got = both({"t": {"type": "terms", "field": "tag"}}, cols, {"tag": ["a", "b"]})
    assert counts(want["t"]) == [("a", 2), ("b", 1)]
    assert got == want


def test_histogram_distinct_buckets_per_doc():
    # doc 0: 1 and 4 share bucket 0 of interval 5 -> once; doc 1: 1 and 7 -> buckets 0 and 1
    cols = one_seg(x=[[1, 4], [1, 7]])
    want, got = both({"h": {"type": "histogram", "field": "x", "interval": 5}}, cols)
    assert counts(want["h"]) == [(0.0, 2), (5.0, 1)]
    assert got == want


def test_histogram_offset_and_negative_value():
    assert R.bucket_id(-0.5, 1, 0.25) == -1  # floor((-0.5 - 0.25) / 1) = floor(-0.75)
    assert R.bucket_id(0.25, 1, 0.25) == 0 and R.bucket_id(0.2, 1, 0.25) == -1
    cols = one_seg(x=[[-0.5], [0.3], [1.25]])
    want, got = both({"h": {"type": "histogram", "field": "x", "interval": 1, "offset": 0.25}}, cols)
    assert counts(want["h"]) == [(-0.75, 1), (0.25, 1), (1.25, 1)]  # key = id * interval + offset
    assert got == want


def test_hard_bounds_skip_a_value():
    cols = one_seg(x=[[1, 50], [12], [200]])
    req = {"h": {"type": "histogram", "field": "x", "interval": 10, "hard_bounds": {"min": 0, "max": 20}}}
    want, got = both(req, cols)
    # 50 and 200 are skipped; min_doc_count defaults to 0 with bounds, zero buckets over the hard bounds
    assert counts(want["h"]) == [(0.0, 1), (10.0, 1), (20.0, 0)]
    assert got == want


def test_missing_on_terms_with_its_own_key_and_with_an_existing_key():
    cols = one_seg(tag=[["a"], [], ["b"], []])
    want, got = both({"t": {"type": "terms", "field": "tag", "missing": "none"}}, cols, {"tag": ["a", "b"]})
    assert counts(want["t"]) == [("none", 2), ("a", 1), ("b", 1)]
    assert got == want
    want, got = both({"t": {"type": "terms", "field": "tag", "missing": "b"}}, cols, {"tag": ["a", "b"]})
    assert counts(want["t"]) == [("b", 3), ("a", 1)]
    assert got == want


def test_missing_on_histogram_and_stats():
    cols = one_seg(x=[[3], [], [8]])
    req = {"h": {"type": "histogram", "field": "x", "interval": 5, "missing": 11},
           "s": {"type": "stats", "field": "x", "missing": -2}}
    want, got = both(req, cols)
    assert counts(want["h"]) == [(0.0, 1), (5.0, 1), (10.0, 1)]
    assert want["s"] == {"type": "stats", "count": 3, "min": -2.0, "max": 8.0, "sum": 9.0, "avg": 3.0}
    assert got == want
    want, got = both({"s": {"type": "stats", "field": "x"}}, cols)
    assert want["s"]["count"] == 2 and want["s"]["sum"] == 11.0
    assert got == want


def test_empty_stats_are_all_zero():
    want, got = both({"s": {"type": "stats", "field": "x"}}, one_seg(x=[[], []]))
    assert want["s"] == {"type": "stats", "count": 0, "min": 0.0, "max": 0.0, "sum": 0.0, "avg": 0.0}
    assert got == want


def test_range_to_is_inclusive_and_ranges_overlap():
    cols = one_seg(x=[[20], [25, 45], [19.5]])
    req = {"r": {"type": "range", "field": "x",
                 "ranges": [{"to": 20}, {"from": 20, "to": 40}, {"from": 40}, {"key": "all", "from": 0}]}}
    want, got = both(req, cols)
    # 20 is in `to: 20` (inclusive) and in `from: 20`; doc 1 is in two ranges by its two values
    assert [b["doc_count"] for b in want["r"]["buckets"]] == [2, 2, 1, 3]
    assert want["r"]["buckets"][0]["key"] == {"from": None, "to": 20} and want["r"]["buckets"][3]["key"] == "all"
    assert got == want


def test_stats_under_terms_for_a_doc_in_two_parent_buckets():
    cols = one_seg(tag=[["a", "b"], ["a"]], x=[[1, 2], [10]])
    req = {"t": {"type": "terms", "field": "tag", "aggs": {"s": {"type": "stats", "field": "x"}}}}
    want, got = both(req, cols, {"tag": ["a", "b"]})
    by = {b["key"]: b for b in want["t"]["buckets"]}
    assert by["a"]["doc_count"] == 2 and by["a"]["aggregations"]["s"]["sum"] == 13.0  # 1 + 2 + 10
    assert by["b"]["doc_count"] == 1 and by["b"]["aggregations"]["s"]["count"] == 2   # doc 0's values again
    assert got == want


def test_terms_tie_is_decided_by_key_string_order():
    cols = one_seg(tag=[["9"], ["10"], ["10"], ["9"], ["2"]])
    want, got = both({"t": {"type": "terms", "field": "tag"}}, cols, {"tag": ["10", "2", "9"]})
    assert counts(want["t"]) == [("10", 2), ("9", 2), ("2", 1)]  # "10" < "9" as strings
    assert got == want


def test_size_and_min_doc_count():
    cols = one_seg(tag=[["a"], ["a"], ["a"], ["b"], ["b"], ["c"]])
    keys = {"tag": ["a", "b", "c"]}
    want, got = both({"t": {"type": "terms", "field": "tag", "size": 1}}, cols, keys)
    assert counts(want["t"]) == [("a", 3)]
    assert got == want
    want, got = both({"t": {"type": "terms", "field": "tag", "min_doc_count": 2}}, cols, keys)
    assert counts(want["t"]) == [("a", 3), ("b", 2)]
    assert got == want


def test_extended_bounds_zero_buckets():
    cols = one_seg(x=[[12], [31]])
    req = {"h": {"type": "histogram", "field": "x", "interval": 10, "extended_bounds": {"min": 0, "max": 45}}}
    want, got = both(req, cols)
    assert counts(want["h"]) == [(0.0, 0), (10.0, 1), (20.0, 0), (30.0, 1), (40.0, 0)]
    assert got == want
    req["h"]["min_doc_count"] = 1
    want, got = both(req, cols)
    assert counts(want["h"]) == [(10.0, 1), (30.0, 1)]
    assert got == want


def test_children_of_every_kind_and_two_segments():
    columns = {"tag": [[["a"], ["b", "a"]], [["b"], []]], "x": [[[1], [7, 8]], [[3], [4]]]}
    req = {"t": {"type": "terms", "field": "tag", "missing": "z",
                 "aggs": {"h": {"type": "histogram", "field": "x", "interval": 5},
                          "r": {"type": "range", "field": "x", "ranges": [{"to": 3}, {"from": 3}]},
                          "s": {"type": "stats", "field": "x"},
                          "u": {"type": "terms", "field": "tag"}}}}
    docs = [(0, 0), (0, 1), (1, 0), (1, 1)]
    want, got = both(req, columns, {"tag": ["a", "b"]}, docs)
    by = {b["key"]: b for b in want["t"]["buckets"]}
    assert by["b"]["doc_count"] == 2 and counts(by["b"]["aggregations"]["h"]) == [(0.0, 1), (5.0, 1)]
    assert by["z"]["aggregations"]["s"]["sum"] == 4.0
    assert got == want


def test_spec_struct_follows_the_request():
    from searchlite_amd import _native as N, aggs as A
    req = {"b": {"type": "range", "field": "x", "ranges": [{"to": 2}, {"from": 2, "to": 5}]},
           "a": {"type": "terms", "field": "tag", "missing": "b",
                 "aggs": {"s": {"type": "stats", "field": "x", "missing": 1.5}}}}
    plan = A.agg_spec(req, {"x": {"id": 4}, "tag": {"id": 7, "keys": ["a", "b"]}})
    sp = plan.spec
    assert sp.n_nodes == 3 and [n["name"] for n in plan.nodes] == ["a", "s", "b"]
    assert (sp.nodes[0].kind, sp.nodes[0].field, sp.nodes[0].parent) == (N.AGG_TERMS, 7, -1)
    assert sp.nodes[0].has_missing == 1 and sp.nodes[0].missing_ord == 1
    assert (sp.nodes[1].kind, sp.nodes[1].parent, sp.nodes[1].missing) == (N.AGG_STATS, 0, 1.5)
    assert sp.nodes[2].n_ranges == 2 and sp.nodes[2].from_[0] == -np.inf and sp.nodes[2].to[1] == 5.0
