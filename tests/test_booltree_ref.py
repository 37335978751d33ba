"""tests/booltree_ref.py, the reference of the nested-matcher tests, against hand-derived cases for each node kind
of QueryEvaluator::matches_node (api/reader.rs:1485-1565), and searchlite_amd/booltree.py's compile_matchers
against it: over 200 random trees the compiled form (the spec's arrays, evaluated as masks) equals the recursive
form doc for doc."""
import numpy as np
import pytest

from searchlite_amd import booltree as BT
from tests import booltree_ref as R
from tests.test_bool_ref import SEG, SEG2, seg_of

NO_TERM = R.NO_TERM
# SEG: 8 docs; term 0 = {0,1,2,3}, term 1 = {2,3,4,5}, term 2 = {3,5,7}, term 3 = {}.  SEG2: 4 docs; 0 = {0,2}, 1 = {1}
T = lambda *ids: {"term": list(ids)}
FILTERS = {0: [np.array([1, 0, 1, 0, 1, 0, 1, 0], bool), None], 1: [np.array([0, 0, 0, 1, 1, 1, 1, 1], bool), np.array([1, 1, 0, 0], bool)]}


def both(d, segs=(SEG,), filters=None):
    """the docs description d accepts per segment — by the recursive form, which the compiled form must equal"""
    segs = list(segs)
    want = R.nested_masks(segs, [d], filters)[0]
    got = R.compiled_masks(segs, BT.compile_matchers([d], len(segs)), filters)[0]
    assert (want is None) == (got is None)
    if want is None:
        return None
    for w, g in zip(want, got):
        assert np.array_equal(w, g), (d, np.nonzero(w)[0], np.nonzero(g)[0])
    return [np.nonzero(w)[0].tolist() for w in want]


ALL = list(range(8))


def test_single_term_and_match_all():
    assert both(T(0)) == [[0, 1, 2, 3]]
    assert both(T(0, 2)) == [[0, 1, 2, 3, 5, 7]]
    assert both("match_all") == [ALL]
    assert both(None) is None
    tree = BT.compile_matchers([T(0), None, "match_all"], 1)
    assert tree["n_offsets"].tolist() == [0, 1, 1, 2] and tree["g_offsets"].tolist() == [0, 1, 1, 1]
    assert tree["e_child"].tolist() == [0] and tree["e_kind"].tolist() == [R.MUST] and tree["n_min_should"].tolist() == [0, 0]


def test_empty_dis_max_is_never_true():
    assert both({"dis_max": []}) == [[]]
    assert both({"bool": {"should": [{"dis_max": []}, T(2)]}}) == [[3, 5, 7]]
    assert both({"bool": {"must": [T(0)], "must_not": [{"dis_max": []}]}}) == [[0, 1, 2, 3]]
    assert both({"dis_max": [T(0), T(2)]}) == [[0, 1, 2, 3, 5, 7]]


def test_query_string():
    assert both({"query_string": {}}) == [[]]                              # no group at all: never true
    assert both({"query_string": {"terms": [], "not": []}}) == [[]]
    assert both({"query_string": {"not": [[2]]}}) == [[0, 1, 2, 4, 6]]    # only not-groups: true where none holds
    assert both({"query_string": {"not": [[2]], "minimum_should_match": 2}}) == [[0, 1, 2, 4, 6]]  # (not looked at)
    assert both({"query_string": {"terms": [[0], [1]]}}) == [[0, 1, 2, 3, 4, 5]]  # unwrap_or(1)
    assert both({"query_string": {"terms": [[0], [1]], "minimum_should_match": 2}}) == [[2, 3]]
    assert both({"query_string": {"terms": [[0], [1]], "minimum_should_match": 0}}) == [ALL]
    assert both({"query_string": {"terms": [[0], [1]], "not": [[2]]}}) == [[0, 1, 2, 4]]
    assert both({"query_string": {"terms": [[0, 2]], "minimum_should_match": 1}}) == [[0, 1, 2, 3, 5, 7]]


def test_default_min_should_rule():
    # no should children: 0
    assert both({"bool": {"must": [T(0)]}}) == [[0, 1, 2, 3]]
    # should children, must and filter both empty: 1
    assert both({"bool": {"should": [T(0), T(2)]}}) == [[0, 1, 2, 3, 5, 7]]
    assert both({"bool": {"should": [T(0)], "must_not": [T(1)]}}) == [[0, 1]]
    # should children beside a must: 0
    assert both({"bool": {"must": [T(0)], "should": [T(2)]}}) == [[0, 1, 2, 3]]
    # should children beside a filter only: 0 — the filter alone decides
    assert both({"bool": {"filter": [0], "should": [T(2)]}}, filters=FILTERS) == [[0, 2, 4, 6]]
    # stated: used as it is, also without should children (nothing can reach it)
    assert both({"bool": {"must": [T(0)], "should": [T(2)], "minimum_should_match": 1}}) == [[3]]
    assert both({"bool": {"must": [T(0)], "minimum_should_match": 1}}) == [[]]
    assert both({"bool": {}}) == [ALL]


def test_filters_and_absent_bitmaps():
    d = {"bool": {"must": [T(1)], "filter": [0, 1]}}
    assert both(d, (SEG, SEG2), FILTERS) == [[4], [1]]  # filter 0 has no bitmap for the second segment: passes all
    d = {"bool": {"must_not": [{"bool": {"filter": [1]}}]}}
    assert both(d, (SEG, SEG2), FILTERS) == [[0, 1, 2], [2, 3]]
    tree = BT.compile_matchers([d], 2)
    assert tree["f_filter"].tolist() == [1] and tree["e_child"].tolist() == [0, 1] and tree["e_kind"].tolist() == [R.MUST, R.MUST_NOT]


def test_must_not_of_a_bool_with_a_must_not():
    inner = {"bool": {"must": [T(0)], "must_not": [T(1)]}}  # {0, 1}
    assert both(inner) == [[0, 1]]
    assert both({"bool": {"must_not": [inner]}}) == [[2, 3, 4, 5, 6, 7]]
    assert both({"bool": {"must": [T(2)], "must_not": [{"bool": {"must_not": [T(1)]}}]}}) == [[3, 5]]  # double negation
    assert both({"bool": {"must_not": [{"bool": {"must_not": [{"bool": {"must_not": [T(0)]}}]}}]}}) == [[4, 5, 6, 7]]


def test_absent_terms_and_segments():
    d = {"bool": {"must": [{"bool": {"must": [T((0, NO_TERM))]}}]}}
    assert both(d, (SEG, SEG2)) == [[0, 1, 2, 3], []]
    d = {"bool": {"must": [T(0)], "should": [{"dis_max": [T((NO_TERM, NO_TERM))]}], "must_not": [{"bool": {"must": [T((NO_TERM, NO_TERM))]}}]}}
    assert both(d, (SEG, SEG2)) == [[0, 1, 2, 3], [0, 2]]
    assert both({"bool": {"must": [T(3)]}}) == [[]]  # an empty list is an absent term


def test_phrase_and_unknown_kinds_are_refused():
    from searchlite_amd import _native as N
    with pytest.raises(N.SlgError) as ei:
        BT.compile_matchers([{"bool": {"must": [{"phrase": [[0, 1]]}]}}], 1)
    assert ei.value.code == N.ERR_UNSUPPORTED
    for bad in ({"nope": []}, "everything", {"term": []}, {"bool": {}, "dis_max": []}):
        with pytest.raises(N.SlgError) as ei:
            BT.compile_matchers([bad], 1)
        assert ei.value.code == N.ERR_INVALID


def test_accept_masks_and_scored_docs():
    queries = [{"bool": {"must_not": [{"dis_max": [T(2)]}]}}, None]
    flt = {0: [np.array([1, 1, 1, 0, 0, 0, 0, 1], bool)]}
    acc = R.accept_masks([SEG], queries, q_filter=np.array([0, 0]), filters=flt)
    assert np.nonzero(acc[0][0])[0].tolist() == [0, 1, 2] and np.nonzero(acc[1][0])[0].tolist() == [0, 1, 2, 7]
    assert R.accept_masks([SEG], queries)[1] == [None]
    offs, terms = np.array([0, 2, 3], np.uint32), np.array([[0], [1], [2]], np.uint32)
    assert R.scored_docs([SEG], offs, terms, queries).tolist() == [4, 3]


def test_200_random_trees_compiled_equals_recursive():
    """fixed seed; depth <= 4, <= 32 leaves, <= 32 nodes; two small segments; filter leaves with and without a
    bitmap: the compiled arrays evaluated as masks equal the recursive matcher doc for doc"""
    rng = np.random.default_rng(20240611)
    vocab = 12
    def small(n):
        return seg_of(n, [sorted(rng.choice(n, size=int(rng.integers(0, n)), replace=False).tolist()) for _ in range(vocab)])
    segs = [small(40), small(23)]
    filters = {0: [rng.random(40) < 0.5, None], 1: [rng.random(40) < 0.7, rng.random(23) < 0.3]}
    shapes = set()
    for i in range(200):
        budget = {"leaves": 32, "nodes": 32}
        d = R.random_tree(rng, vocab, 4, budget, filter_ids=(0, 1))
        tree = BT.compile_matchers([None, d], 2)
        nl = int(tree["g_offsets"][2] - tree["g_offsets"][1]) + int(tree["f_offsets"][2] - tree["f_offsets"][1])
        nn = int(tree["n_offsets"][2] - tree["n_offsets"][1])
        assert nl <= 32 and 1 <= nn <= 32, (i, nl, nn)
        shapes.add((nl > 8, nn > 4))
        want = R.nested_masks(segs, [None, d], filters)
        got = R.compiled_masks(segs, tree, filters)
        assert want[0] is None and got[0] is None
        for s in range(2):
            assert np.array_equal(want[1][s], got[1][s]), (i, d)
    assert len(shapes) >= 3  # small and large trees both occur
