"""tests/agg_values_ref.py against numpy and against the reference's own test, and aggs.shape on hand-made value
tables (no device)."""
import math

import numpy as np
import pytest

from tests import agg_values_ref as V


def ulps(a, b):
    """distance of two finite doubles in units of the spacing at the larger one"""
    if a == b:
        return 0.0
    return abs(a - b) / np.spacing(max(abs(a), abs(b)))


def test_percentile_against_numpy_linear():
    """numpy's method="linear" interpolates the same two order statistics, but as lo + (hi - lo) * w (one rounding
    of the difference, one of the product, one of the sum) where the reference computes lo * (1 - w) + hi * w
    (:537).  Both are within a few roundings of lo + (hi - lo) w; when lo and hi are of similar size, as here
    (uniform values in [1, 2): every term is in [0, 2] and the result in [1, 2)), each rounding is at most half
    an ulp of the result, so the two differ by at most 1/2 * (3 + 4) < 4 ulps.  Observed: at most 1 ulp."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for n in (1, 2, 3, 10, 255, 256, 257, 1000):
        vals = [float(x) for x in rng.random(n) + 1.0]
        for p in [0.0, 100.0, 50.0, 1.0, 99.0] + [float(x) for x in rng.random(20) * 100.0]:
            want = float(np.percentile(np.array(vals), p, method="linear"))
            got = V.percentile(vals, p)
            worst = max(worst, ulps(got, want))
            assert ulps(got, want) <= 4, (n, p, got, want)
    print("largest distance from numpy:", worst, "ulps")


def test_order_statistics_are_exact_when_rank_is_whole():
    vals = [10.0, 30.0, 20.0, 50.0, 40.0]
    for p, want in [(0, 10.0), (25, 20.0), (50, 30.0), (75, 40.0), (100, 50.0)]:
        assert V.percentile(vals, float(p)) == want  # (p / 100) * 4 is a whole number exactly: low == high
    # not every "whole" rank is one in f64: (7 / 100) * 100 = 7.000000000000001, between elements 7 and 8
    assert V.rank_low_high(101, 7.0)[1:] == (7, 8)


def test_reference_own_small_sample():
    """aggs/mod.rs tests::quantile_state_handles_small_samples (:3520-3528)"""
    vals = [1.0, 2.0, 3.0, 4.0]
    assert abs(V.percentile(vals, 50.0) - 2.5) < 1e-6
    assert abs(V.percentile_rank(vals, 2.0) - 50.0) < 1e-6


def test_more_than_256_values_use_the_exact_formula():
    """the deviation: no t-digest; 1000 values 0 .. 999, p = 50 -> rank 499.5 -> exactly 499.5"""
    vals = [float(x) for x in range(1000)]
    assert len(vals) > V.EXACT_LIMIT
    assert V.percentile(vals, 50.0) == 499.5
    assert V.percentile_rank(vals, 249.0) == 25.0


def test_empty_and_out_of_range_percents():
    assert V.percentile([], 50.0) == 0.0 and V.percentile_rank([], 1.0) == 0.0
    vals = [3.0, 1.0, 2.0]
    assert V.percentile(vals, -5.0) == 1.0 and V.percentile(vals, 0.0) == 1.0  # clamp(0, 100)
    assert V.percentile(vals, 250.0) == 3.0 and V.percentile(vals, 100.0) == 3.0
    assert V.rank_low_high(3, -5.0) == (0.0, 0, 0) and V.rank_low_high(3, 1e9) == (2.0, 2, 2)
    assert V.rank_low_high(1, 50.0) == (0.0, 0, 0) and V.rank_low_high(2, 50.0) == (0.5, 0, 1)


COLS = {"x": [[[0.0, -0.0], [1.5, 1.5, 1.5], [], [-0.0]], [[2.0], []]],
        "k": [[["a", "a", "b"], [], ["c"], []], [["a"], []]]}
ALL = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1)]


def test_cardinality_zero_signs_duplicates_and_missing():
    card = lambda body, docs=ALL: V.respond_one(body, V.run({"c": body}, COLS, docs)[("c",)])["value"]
    assert card({"type": "cardinality", "field": "x"}) == 4            # -0.0, 0.0, 1.5, 2.0: the zeros are two
    assert card({"type": "cardinality", "field": "x"}, [(0, 1)]) == 1  # a value three times in one doc
    assert card({"type": "cardinality", "field": "x", "missing": 1.5}) == 4   # a missing the column holds
    assert card({"type": "cardinality", "field": "x", "missing": 7.0}) == 5   # and one it does not
    assert card({"type": "cardinality", "field": "x", "missing": 7.0}, [(0, 0)]) == 2  # no doc without a value
    assert card({"type": "cardinality", "field": "x"}, []) == 0
    assert card({"type": "cardinality", "field": "k"}) == 3
    assert card({"type": "cardinality", "field": "k", "missing": "zz"}) == 4
    assert card({"type": "cardinality", "field": "k", "missing": "a"}) == 3


def test_percentile_ranks_counts_are_inclusive():
    body = {"type": "percentile_ranks", "field": "x", "values": [1.5, -1.0, 9.0, 0.0]}
    st = V.run({"r": body}, COLS, ALL)[("r",)]
    assert V.cells(body, st) == [7, 6, 0, 7, 3]  # -0.0 <= 0.0: the three zeros
    assert V.respond_one(body, st)["values"] == {"1.5": 6 / 7 * 100.0, "-1": 0.0, "9": 100.0, "0": 3 / 7 * 100.0}


def test_children_collect_once_per_parent_bucket():
    req = {"t": {"type": "terms", "field": "k", "missing": "none",
                 "aggs": {"c": {"type": "cardinality", "field": "x"},
                          "r": {"type": "percentile_ranks", "field": "x", "values": [1.0]}}}}
    st = V.run(req, COLS, ALL)
    assert len(st[("t", "a", "c")]["set"]) == 3 and st[("t", "a", "r")]["values"] == [0.0, -0.0, 2.0]
    assert len(st[("t", "b", "c")]["set"]) == 2           # doc (0, 0) is in a ONCE and in b
    assert st[("t", "none", "r")]["values"] == [1.5, 1.5, 1.5, -0.0]   # docs (0, 1), (0, 3), (1, 1)
    assert V.strip(req) == {"t": {"type": "terms", "field": "k", "missing": "none"}}


def test_dense_value_tables():
    from searchlite_amd import aggs as A
    req = {"t": {"type": "terms", "field": "k", "aggs": {"c": {"type": "cardinality", "field": "x"}}},
           "p": {"type": "percentiles", "field": "x", "percents": [50, 100]}}
    plan = A.agg_spec(req, {"k": {"id": 0, "keys": ["a", "b", "c"]}, "x": {"id": 1}})
    assert [n["name"] for n in plan.nodes] == ["p", "t", "c"]
    lay = V.ref_layout(plan.nodes, COLS, {"k": ["a", "b", "c"]})
    assert [(x["parent_rows"], x["rows"]) for x in lay] == [(1, 5), (1, 3), (3, 1)]
    tabs = V.dense(plan.nodes, lay, V.run(req, COLS, ALL), {"k": ["a", "b", "c"]})
    assert tabs[1] is None and tabs[2].tolist() == [[3], [2], [0]]
    n, lo50, hi50, lo100, hi100 = (int(x) for x in tabs[0][0])
    f = lambda b: float(np.uint64(b).view(np.float64))
    assert n == 7 and f(lo50) == 1.5 and f(hi50) == 1.5 and f(lo100) == 2.0 and f(hi100) == 2.0


# ---- aggs.shape on hand-made value tables ----------------------------------------------------------------
def test_rust_float_keys():
    from searchlite_amd import aggs as A
    for x, s in [(50.0, "50"), (99.9, "99.9"), (1.0, "1"), (0.5, "0.5"), (-0.0, "-0"), (1e21, "1" + "0" * 21),
                 (1e-7, "0.0000001"), (100.0, "100"), (2.5e-3, "0.0025")]:
        assert A.rust_f64(x) == s and V.rust_f64(x) == s


def test_shape_of_the_three_value_types():
    from searchlite_amd import aggs as A
    bits = lambda x: int(np.float64(x).view(np.uint64))
    req = {"c": {"type": "cardinality", "field": "x"},
           "p": {"type": "percentiles", "field": "x", "percents": [50, 99.9]},
           "d": {"type": "percentiles", "field": "x"},
           "r": {"type": "percentile_ranks", "field": "x", "values": [2.0, 10]}}
    plan = A.agg_spec(req, {"x": {"id": 3}})
    assert [n["name"] for n in plan.nodes] == ["c", "d", "p", "r"]
    sp = plan.spec
    assert [sp.nodes[i].kind for i in range(4)] == [4, 5, 5, 6]
    assert sp.nodes[1].n_ranges == 7 and list(sp.nodes[1].from_[:7]) == A.DEFAULT_PERCENTS
    assert sp.nodes[2].n_ranges == 2 and list(sp.nodes[2].from_[:2]) == [50.0, 99.9]
    assert sp.nodes[3].n_ranges == 2 and list(sp.nodes[3].from_[:2]) == [2.0, 10.0]
    # n = 4 values 1, 2, 3, 4: p50 -> rank 1.5 (2, 3); p99.9 -> rank 2.997 (3, 4); the defaults likewise
    srt = [1.0, 2.0, 3.0, 4.0]

    def pct_row(percents):
        row = [4]
        for p in percents:
            _, lo, hi = V.rank_low_high(4, p)
            row += [bits(srt[lo]), bits(srt[hi])]
        return np.array([[row]], dtype=np.uint64)

    tables = [np.array([[[17]]], np.uint64), pct_row(A.DEFAULT_PERCENTS), pct_row([50.0, 99.9]),
              np.array([[[4, 2, 4]]], np.uint64)]
    layout = [dict(first_id=0)] * 4
    out = A.shape(plan, layout, tables, 0)
    assert out["c"] == {"type": "cardinality", "value": 17}
    assert out["p"]["type"] == "percentiles" and list(out["p"]["values"]) == ["50", "99.9"]
    assert out["p"]["values"]["50"] == 2.5 and out["p"]["values"]["99.9"] == V.percentile(srt, 99.9)
    assert list(out["d"]["values"]) == ["1", "5", "25", "50", "75", "95", "99"]
    assert out["d"]["values"] == {V.rust_f64(p): V.percentile(srt, p) for p in A.DEFAULT_PERCENTS}
    assert out["r"] == {"type": "percentile_ranks", "values": {"2": 50.0, "10": 100.0}}
    # n == 0: zeros everywhere
    empty = [np.zeros_like(t) for t in tables]
    out = A.shape(plan, layout, empty, 0)
    assert out["c"]["value"] == 0 and set(out["p"]["values"].values()) == {0.0}
    assert set(out["r"]["values"].values()) == {0.0}


def test_value_children_and_refused_nesting():
    from searchlite_amd import aggs as A
    fields = {"k": {"id": 0, "keys": ["a", "b"]}, "x": {"id": 1}}
    req = {"t": {"type": "terms", "field": "k", "aggs": {"c": {"type": "cardinality", "field": "k", "missing": "b"},
                                                        "u": {"type": "cardinality", "field": "k", "missing": "zz"}}}}
    plan = A.agg_spec(req, fields)
    c, u = plan.spec.nodes[1], plan.spec.nodes[2]
    assert (c.kind, c.parent, c.has_missing, c.missing_ord) == (4, 0, 1, 1)
    assert (u.has_missing, u.missing_ord) == (1, 2)  # a key of its own: n_ords
    tables = [np.array([[[5, 2]]], np.uint64), np.array([[[2], [1]]], np.uint64), np.array([[[3], [1]]], np.uint64)]
    out = A.shape(plan, [dict(first_id=0)] * 3, tables, 0)
    assert out["t"]["buckets"][0] == {"key": "a", "doc_count": 5,
                                      "aggregations": {"c": {"type": "cardinality", "value": 2},
                                                       "u": {"type": "cardinality", "value": 3}}}
    with pytest.raises(ValueError):
        A.agg_spec({"c": {"type": "cardinality", "field": "x", "aggs": {"s": {"type": "stats", "field": "x"}}}}, fields)
