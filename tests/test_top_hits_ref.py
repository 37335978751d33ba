"""tests/top_hits_ref.py against hand-derived tables: the reference's own two tests (tests/aggregation_bounds.rs:430-514),
`from` at and beyond the collected docs, a multi-valued doc as a hit of two buckets, ties by (segment, doc), Missing
after every value in both orders, the 0.0 score of a field sort without `_score`, and how the one-collector lists the
device returns relate to the reference's per-segment collect and merge."""
import numpy as np
import pytest

from tests import top_hits_ref as T

F32 = np.float32


def test_reference_four_docs_size_two():
    """top_hits_returns_requested_docs: four docs match, size 2, empty sort -> total 4, two hits, `_score` desc"""
    hits = [(0, d, F32(s)) for d, s in enumerate((0.5, 0.75, 0.25, 0.75))]
    total, best = T.one_list(hits, 2, 0, [], {})
    assert total == 4 and best == [(0, 1, F32(0.75)), (0, 3, F32(0.75))]  # the tie: doc asc
    assert T.per_segment(hits, 2, 0, [], {}) == (total, best)


def test_reference_priority_sort():
    """top_hits_applies_sort_spec: a numeric field desc gives the order, whatever the scores"""
    fields = {"priority": ([[[1], [3], [2]]], False)}
    hits = [(0, 0, F32(9.0)), (0, 1, F32(1.0)), (0, 2, F32(5.0))]
    total, best = T.one_list(hits, 2, 0, [("priority", "desc")], fields)
    assert total == 3 and [d for _, d, _ in best] == [1, 2]
    total, best = T.one_list(hits, 3, 0, [("priority", "asc")], fields)
    assert [d for _, d, _ in best] == [0, 2, 1]


@pytest.mark.parametrize("frm,size,want", [(0, 2, [0, 1]), (1, 2, [1, 2]), (2, 2, [2]), (3, 2, []), (9, 2, []),
                                           (2, 1, [2]), (0, 5, [0, 1, 2])])
def test_from_at_and_beyond_the_collected(frm, size, want):
    """three docs in score order 0, 1, 2: the rows [from, from + size) of the limit best; total counts every doc"""
    hits = [(0, 2, F32(1.0)), (0, 0, F32(3.0)), (0, 1, F32(2.0))]
    total, best = T.one_list(hits, size, frm, [], {})
    assert total == 3 and [d for _, d, _ in best] == want
    assert T.per_segment(hits, size, frm, [], {}) == (total, best)  # (one segment: the merge never runs)


def test_limit_keeps_the_best_whatever_the_arrival_order():
    rng = np.random.default_rng(7)
    hits = [(0, d, F32(d % 11)) for d in range(40)]
    want = sorted(hits, key=lambda h: (-float(h[2]), h[1]))[3:8]
    for _ in range(5):
        order = [hits[i] for i in rng.permutation(len(hits))]
        assert T.one_list(order, 5, 3, [], {}) == (40, want)


def test_multi_valued_doc_is_a_hit_of_two_buckets():
    """terms on a column where doc 1 holds two keys and doc 2 the same key twice: doc 1 is in both lists, doc 2 once"""
    columns = {"kw": [[["a"], ["a", "b"], ["b", "b"], []]]}
    body = {"type": "terms", "field": "kw", "missing": "none"}
    lay = {"rows": 3, "first_id": 0}
    hits = [(0, d, F32(4 - d)) for d in range(4)]
    lists = T.lists_of(body, lay, hits, columns, {}, {"kw": ["a", "b"]})
    assert [[d for _, d, _ in lst] for lst in lists] == [[0, 1], [1, 2], [3]]  # the missing row last
    nodes = [dict(parent=body, parent_lay=lay, **{"from": 0}, size=2, sort=[])]
    got, totals = T.expected(nodes, None, [hits], columns, {}, {"kw": ["a", "b"]}, {})
    assert got[0]["doc"][0].tolist() == [[0, 1], [1, 2], [3, 0]] and got[0]["count"][0].tolist() == [2, 2, 1]
    assert totals[0][0].tolist() == [2, 2, 1]


def test_overlapping_ranges_hold_one_doc_twice():
    columns = {"x": [[[1.0], [5.0], [9.0]]]}
    body = {"type": "range", "field": "x", "ranges": [{"to": 5.0}, {"from": 5.0}]}
    lists = T.lists_of(body, {"rows": 2, "first_id": 0}, [(0, d, F32(1.0)) for d in range(3)], columns, {}, {})
    assert [[d for _, d, _ in lst] for lst in lists] == [[0, 1], [1, 2]]  # (`to` is inclusive)


def test_ties_fall_to_segment_then_doc():
    fields = {"same": ([[[5]] * 3, [[5]] * 3], False)}
    hits = [(1, 0, F32(1.0)), (0, 2, F32(2.0)), (1, 2, F32(9.0)), (0, 0, F32(0.5)), (0, 1, F32(3.0)), (1, 1, F32(4.0))]
    _, best = T.one_list(hits, 4, 1, [("same", "asc")], fields)
    assert [(s, d) for s, d, _ in best] == [(0, 1), (0, 2), (1, 0), (1, 1)]
    _, best = T.one_list(hits, 6, 0, [("same", "desc")], fields)
    assert [(s, d) for s, d, _ in best] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]


@pytest.mark.parametrize("order,want", [("asc", [2, 0, 1, 3]), ("desc", [0, 2, 1, 3])])
def test_missing_after_every_value_in_both_orders(order, want):
    """docs 1 and 3 hold no value: behind the others in both orders, doc asc among themselves; a doc with two values
    sorts by its smallest (asc) or largest (desc)"""
    fields = {"v": ([[[7.5], [], [-2.0, 7.0], []]], True)}
    hits = [(0, 3, F32(1.0)), (0, 1, F32(1.0)), (0, 0, F32(1.0)), (0, 2, F32(1.0))]
    _, best = T.one_list(hits, 4, 0, [("v", order)], fields)
    assert [d for _, d, _ in best] == want


def test_score_is_zero_under_a_field_sort_without_score():
    """the collector is handed ScoreMode::MatchOnly's 0.0: the hits report it, and a `_score` part ties everywhere"""
    fields = {"v": ([[[3], [1], [2]]], False)}
    hits = [(0, d, F32(10 + d)) for d in range(3)]
    nodes = [dict(parent=None, size=3, sort=[("_score", "desc"), ("v", "asc")], **{"from": 0})]
    got, _ = T.expected(nodes, None, [hits], {}, {}, {}, fields, match_only=True)
    assert got[0]["doc"][0, 0].tolist() == [1, 2, 0] and not got[0]["score"].any()
    got, _ = T.expected(nodes, None, [hits], {}, {}, {}, fields)
    assert got[0]["doc"][0, 0].tolist() == [2, 1, 0] and got[0]["score"][0, 0].tolist() == [12.0, 11.0, 10.0]


def random_case(rng):
    n_segs = int(rng.integers(1, 4))
    n_docs = [int(rng.integers(0, 30)) for _ in range(n_segs)]
    fields = {"a": ([[[int(rng.integers(0, 4))] if rng.random() < 0.8 else [] for _ in range(n)] for n in n_docs], False),
              "b": ([[[float(v) for v in rng.integers(-3, 4, int(rng.integers(0, 3)))] for _ in range(n)]
                     for n in n_docs], True)}
    hits = [(s, d, F32(rng.integers(0, 5)) / F32(4)) for s, n in enumerate(n_docs) for d in range(n) if rng.random() < 0.7]
    hits = [hits[i] for i in rng.permutation(len(hits))]
    sorts = ([], [("a", "asc")], [("b", "desc"), ("_score", "asc")], [("_score", "desc"), ("a", "desc")],
             [("a", "asc"), ("b", "asc"), ("_score", "desc"), ("a", "desc")])
    return hits, fields, sorts[int(rng.integers(0, len(sorts)))]


def test_per_segment_collect_then_merge_equals_one_collector_at_from_zero():
    """the property the device's "all segments feed one collector" rests on: with from = 0 the merged per-segment
    lists are the one collector's, on random inputs; the totals agree for every from"""
    rng = np.random.default_rng(20261020)
    for _ in range(300):
        hits, fields, sort = random_case(rng)
        size = int(rng.integers(1, 9))
        assert T.per_segment(hits, size, 0, sort, fields) == T.one_list(hits, size, 0, sort, fields)
        frm = int(rng.integers(1, 6))
        assert T.per_segment(hits, size, frm, sort, fields)[0] == T.one_list(hits, size, frm, sort, fields)[0] == len(hits)
        one_seg = [h for h in hits if h[0] == 0]
        assert T.per_segment(one_seg, size, frm, sort, fields) == T.one_list(one_seg, size, frm, sort, fields)


def test_from_is_applied_per_segment_and_again_in_the_merge():
    """What the reference does with from > 0 over two segments, by hand.  Scores 6 .. 1 alternate between the
    segments; from 1, size 2.  One collector: the limit 3 best are 6, 5, 4 and the rows [1, 3) are 5, 4.  The
    reference: segment 0 keeps 6, 4, 2 and finishes with 4, 2; segment 1 keeps 5, 3, 1 and finishes with 3, 1; the
    merge keeps the 3 best of {4, 2, 3, 1} = 4, 3, 2 and slices at from again: 3, 2.  The device returns the one
    collector's rows (include/searchlite_gpu.h); this test pins the difference so that nobody takes it for an accident."""
    hits = [(s, d, F32(6 - (2 * d + s))) for d in range(3) for s in range(2)]
    assert [float(h[2]) for h in sorted(hits, key=lambda h: -float(h[2]))] == [6, 5, 4, 3, 2, 1]
    total, best = T.one_list(hits, 2, 1, [], {})
    assert total == 6 and [float(sc) for _, _, sc in best] == [5.0, 4.0]
    total, best = T.per_segment(hits, 2, 1, [], {})
    assert total == 6 and [float(sc) for _, _, sc in best] == [3.0, 2.0]
