"""tests/phrase_ref.py against the reference's own unit cases (query/phrase.rs:55-116), hand-derived cases of the
definition, the greedy chain test against the exhaustive one, the clause masks over term and phrase groups, and
the host pieces that feed positions in: SegmentBuilder's positions and parse_query_string."""
import numpy as np
import pytest

from tests import bool_ref as B
from tests import phrase_ref as P

MUST, SHOULD, MUST_NOT = P.MUST, P.SHOULD, P.MUST_NOT
BOTH = (P.matches, P.matches_greedy)


@pytest.mark.parametrize("m", BOTH)
def test_the_references_unit_cases(m):
    assert m([[1, 4], [2], [3]], 0)                      # matches_consecutive_positions
    assert not m([[1], [3]], 0)                          # rejects_non_consecutive_positions
    assert not m([[1], [4], [6]], 0) and m([[1], [4], [6]], 3)  # allows_sloppy_phrase: gaps 2 + 1


@pytest.mark.parametrize("m", BOTH)
def test_hand_derived_cases(m):
    # an empty position list fails the variant, also for n = 1
    assert not m([[]], 0) and not m([[]], 5) and m([[7]], 0)
    assert not m([[1], []], 9) and not m([[], [2]], 9)
    # a repeated list needs two distinct positions
    assert not m([[5], [5]], 0) and not m([[5], [5]], 100)
    assert m([[5, 6], [5, 6]], 0) and not m([[5, 7], [5, 7]], 0) and m([[5, 7], [5, 7]], 1)
    # equal positions in two lists are not increasing
    assert not m([[3], [3]], 10) and not m([[3], [2]], 10)
    # slop exactly enough and one short: gaps (4 - 1 - 1) + (9 - 4 - 1) = 6
    assert m([[1], [4], [9]], 6) and not m([[1], [4], [9]], 5)
    # a first start that fails where a later one succeeds
    assert m([[1, 10], [11]], 0) and not m([[1, 9], [11]], 0)
    # a match that must skip positions <= the previous pick
    assert m([[10], [2, 5, 10, 11]], 0) and not m([[10], [2, 5, 10]], 3)
    assert m([[4], [1, 2, 3, 5], [1, 5, 6]], 0)
    # duplicates inside a list (non-decreasing) change nothing
    assert m([[2, 2], [3, 3]], 0) and not m([[2, 2], [2, 2]], 4)
    # the largest slop the ABI takes
    top = 2 ** 31 - 1 - 8  # the gap between positions 0 and top + 1 is top
    assert m([[0], [top + 1]], top) and not m([[0], [top + 1]], top - 1)


def test_greedy_equals_exhaustive_on_random_small_cases():
    rng = np.random.default_rng(3)
    n_match = 0
    for _ in range(4000):
        n = int(rng.integers(1, 5))
        lists = [sorted(rng.integers(0, 12, size=int(rng.integers(0, 7))).tolist()) for _ in range(n)]
        if rng.random() < 0.2 and n > 1:
            lists[int(rng.integers(1, n))] = list(lists[0])  # the same list twice
        slop = int(rng.integers(0, 4))
        want = P.matches(lists, slop)
        assert P.matches_greedy(lists, slop) == want, (lists, slop)
        n_match += want
    assert 500 < n_match < 3500  # both outcomes are exercised


def tokens_world():
    # vocabulary: 0 a, 1 b, 2 c, 3 d;   docs as token sequences
    docs = [[0, 1, 2], [0, 2, 1], [1, 0, 0], [3], [0, 3, 1], [0]]
    return P.segment_from_tokens(docs, 4, extra_postings={3: [5]})


def test_segment_from_tokens_agrees_with_itself():
    seg = tokens_world()
    assert seg.postings(0)[0].tolist() == [0, 1, 2, 4, 5] and seg.postings(0)[1].tolist() == [1, 1, 2, 1, 1]
    assert P.doc_positions(seg, 0, 2) == [1, 2] and P.doc_positions(seg, 1, 4) == [2]
    assert P.doc_positions(seg, 3, 5) == [] and P.doc_positions(seg, 3, 0) is None
    assert int(seg.pos_offsets[-1]) == len(seg.positions) == 14 and len(seg.pos_offsets) == seg.n_postings + 1


def test_clause_masks_over_term_and_phrase_groups():
    seg = tokens_world()
    bare = tokens_world()
    bare.pos_offsets = bare.positions = None
    q = lambda phrases, ms=0: P.phrases_of([(phrases, ms)], 1)
    mask = lambda ph, cl=None, s=seg: P.clause_masks([s], cl, ph)[0][0].nonzero()[0].tolist()
    assert mask(q([(MUST, 0, [[0, 1]])])) == [0]                    # "a b"
    assert mask(q([(MUST, 1, [[0, 1]])])) == [0, 1, 4]              # slop 1
    assert mask(q([(MUST, 0, [[0, 0]])])) == [2]                    # "a a": two occurrences
    assert mask(q([(MUST, 0, [[3]])])) == [3, 4]                    # doc 5's posting of d has no position
    assert mask(q([(MUST_NOT, 0, [[0, 1]])])) == [1, 2, 3, 4, 5]
    assert mask(q([(MUST, 0, [[2, 0], [0, 2]])])) == [1]            # only the second variant matches
    assert mask(q([(MUST, 0, [[P.NO_TERM, 1]])])) == []             # every variant dropped: MUST rejects all
    assert mask(q([(MUST_NOT, 0, [[P.NO_TERM, 1]])])) == [0, 1, 2, 3, 4, 5]
    assert mask(q([(MUST, 0, [])])) == [] and mask(q([(SHOULD, 0, [])], 0)) == [0, 1, 2, 3, 4, 5]
    assert mask(q([(MUST, 0, [[0]])]), s=bare) == []                # no positions: no phrase holds a doc
    assert P.clause_masks([seg], None, q([]))[0] is None            # no group: untouched
    # min_should counts term and phrase SHOULD groups together; phrase groups are numbered after term groups
    cl = B.clauses_of([([(SHOULD, [2]), (MUST_NOT, [3])], 0)], 1)
    del cl["q_min_should"]
    ph = lambda ms: q([(SHOULD, 0, [[0, 1]]), (SHOULD, 0, [[1, 0]])], ms)
    assert mask(ph(0), cl) == [0, 1, 2] and mask(ph(1), cl) == [0, 1, 2]
    assert mask(ph(2), cl) == [0] and mask(ph(3), cl) == [] and mask(ph(4), cl) == []


def test_segment_builder_records_positions():
    from searchlite_amd.segment import SegmentBuilder
    sb = SegmentBuilder(["body", "tags"])
    sb.add_document("a", {"body": "olive oil and olive", "tags": ["x y", "", "z x"]})
    sb.add_document("b", {"body": "oil"})
    seg = sb.build()
    pos = lambda key, d: P.doc_positions(seg, seg.term_id(key), d)
    assert pos("body:olive", 0) == [0, 3] and pos("body:oil", 0) == [1] and pos("body:oil", 1) == [0]
    # multi-valued: values run on without a gap, an empty value leaves a gap of one (index/segment.rs:664-692)
    assert pos("tags:x", 0) == [0, 4] and pos("tags:y", 0) == [1] and pos("tags:z", 0) == [3]
    assert int(seg.pos_offsets[-1]) == int(seg.tfs.sum()) == len(seg.positions)


def test_parse_query_string():
    from searchlite_amd.segment import parse_query_string, parse_query_terms
    w, n, p = parse_query_string('title:Rust body:safety -noise "body:memory safety"', "body")
    assert w == [("title", "Rust"), ("body", "safety")] and n == [("body", "noise")] and p == [("body", ["memory", "safety"])]
    assert parse_query_string('"olive oil" pasta', "body") == ([("body", "pasta")], [], [("body", ["olive", "oil"])])
    assert parse_query_string('a "b c', "f") == ([("f", "a")], [], [])           # an unclosed quote drops the rest
    assert parse_query_string('"" x "a:b:c d"', "f") == ([("f", "x")], [], [("a", ["b:c", "d"])])
    assert parse_query_string('"not-a-field:x"', "f")[2] == [("f", ["not-a-field:x"])]
    with pytest.raises(ValueError):
        parse_query_terms('"olive oil" pasta', "body")
