"""tests/bool_ref.py, the reference of the boolean-query tests, against hand-derived cases: the pass mask of
every clause kind alone, a two-term group, terms absent from a segment under MUST and MUST_NOT, min_should 0, 1,
2 and above the group count, and a query without a clause table."""
import numpy as np

from tests import bool_ref as B

NO_TERM = B.NO_TERM


def seg_of(n_docs, lists):
    from searchlite_amd.segment import Segment
    offs = np.zeros(len(lists) + 1, np.uint64)
    offs[1:] = np.cumsum([len(l) for l in lists])
    docs = np.array([d for l in lists for d in l], np.uint32)
    return Segment(n_docs=n_docs, term_offsets=offs, doc_ids=docs, tfs=np.ones(len(docs), np.uint32),
                   field_doc_len=[np.ones(n_docs, np.float32)], field_avgdl=np.ones(1, np.float32),
                   docs=float(n_docs))


# 8 docs; term 0 = {0,1,2,3}, term 1 = {2,3,4,5}, term 2 = {3,5,7}, term 3 = {} (an empty list)
SEG = seg_of(8, [[0, 1, 2, 3], [2, 3, 4, 5], [3, 5, 7], []])
# a second segment of 4 docs; term 0 = {0, 2}, term 1 = {1}
SEG2 = seg_of(4, [[0, 2], [1]])


def mask(groups, min_should, segs=(SEG,)):
    m = B.clause_masks(list(segs), B.clauses_of([(groups, min_should)], len(segs)))[0]
    return [np.nonzero(x)[0].tolist() for x in m]


def test_each_kind_alone():
    assert mask([(B.MUST, [0])], 0) == [[0, 1, 2, 3]]
    assert mask([(B.MUST_NOT, [0])], 0) == [[4, 5, 6, 7]]
    assert mask([(B.SHOULD, [0])], 1) == [[0, 1, 2, 3]]
    assert mask([(B.SHOULD, [0])], 0) == [list(range(8))]  # no should requirement: every doc passes


def test_all_three_kinds():
    assert mask([(B.MUST, [0]), (B.MUST_NOT, [2]), (B.SHOULD, [1])], 1) == [[2]]
    assert mask([(B.MUST, [0]), (B.MUST, [1])], 0) == [[2, 3]]


def test_two_term_group_is_any_of():
    assert mask([(B.MUST, [0, 2])], 0) == [[0, 1, 2, 3, 5, 7]]
    assert mask([(B.MUST_NOT, [0, 2])], 0) == [[4, 6]]
    assert mask([(B.SHOULD, [0, 2]), (B.SHOULD, [1])], 2) == [[2, 3, 5]]


def test_absent_terms():
    # a MUST group whose terms are all absent from a segment rejects every doc of it; present elsewhere it holds
    assert mask([(B.MUST, [(0, NO_TERM)])], 0, (SEG, SEG2)) == [[0, 1, 2, 3], []]
    assert mask([(B.MUST, [(NO_TERM, 1)])], 0, (SEG, SEG2)) == [[], [1]]
    assert mask([(B.MUST, [3])], 0) == [[]]  # an empty list is an absent term
    # one absent term of a two-term MUST group: the other decides
    assert mask([(B.MUST, [(NO_TERM, 0), (2, NO_TERM)])], 0, (SEG, SEG2)) == [[3, 5, 7], [0, 2]]
    # an absent MUST_NOT term rejects nothing
    assert mask([(B.MUST_NOT, [(0, NO_TERM)])], 0, (SEG, SEG2)) == [[4, 5, 6, 7], [0, 1, 2, 3]]
    assert mask([(B.MUST_NOT, [(NO_TERM, NO_TERM)])], 0, (SEG, SEG2)) == [list(range(8)), list(range(4))]


def test_min_should():
    three = [(B.SHOULD, [0]), (B.SHOULD, [1]), (B.SHOULD, [2])]
    assert mask(three, 0) == [list(range(8))]
    assert mask(three, 1) == [[0, 1, 2, 3, 4, 5, 7]]
    assert mask(three, 2) == [[2, 3, 5]]
    assert mask(three, 3) == [[3]]
    assert mask(three, 4) == [[]]  # more than the query has SHOULD groups: nothing
    # MUST and MUST_NOT groups do not count as should
    assert mask([(B.MUST, [0]), (B.SHOULD, [1])], 2) == [[]]


def test_empty_clause_table_and_mixed_batch():
    cl = B.clauses_of([([], 0), ([(B.MUST, [2])], 0), ([], 5)], 1)
    m = B.clause_masks([SEG], cl)
    assert m[0] is None and m[2] is None  # untouched, whatever min_should says
    assert np.nonzero(m[1][0])[0].tolist() == [3, 5, 7]
    assert cl["c_offsets"].tolist() == [0, 0, 1, 1] and cl["g_offsets"].tolist() == [0, 0, 1, 1]


def test_accept_masks_and_scored_docs():
    cl = B.clauses_of([([(B.MUST_NOT, [2])], 0), ([], 0)], 1)
    flt = {0: [np.array([1, 1, 1, 0, 0, 0, 0, 1], bool)]}
    acc = B.accept_masks([SEG], cl, q_filter=np.array([0, 0]), filters=flt)
    assert np.nonzero(acc[0][0])[0].tolist() == [0, 1, 2]      # not {3,5,7}, and the filter
    assert np.nonzero(acc[1][0])[0].tolist() == [0, 1, 2, 7]   # no clause table: the filter alone
    acc = B.accept_masks([SEG], cl)
    assert acc[1] == [None]
    # scored lists: query 0 scores terms 0 and 1 ({0..5}), minus {3, 5}; query 1 scores term 2, untouched
    offs, terms = np.array([0, 2, 3], np.uint32), np.array([[0], [1], [2]], np.uint32)
    assert B.scored_docs([SEG], offs, terms, cl).tolist() == [4, 3]
