"""tests/term_buckets_ref.py against answers derived by hand from the reference's text (query/aggs/mod.rs:131-359,
2110-2181, 2395-2424, 2515-2595): what the GPU tests take as expected values is checked here first."""
from tests import term_buckets_ref as R


def world(*segs):
    """segs: per segment a list of per-doc value lists -> (cols, n_docs)"""
    return {"f": [list(s) for s in segs]}, [len(s) for s in segs]


def all_docs(n_docs):
    return [(s, d) for s, n in enumerate(n_docs) for d in range(n)]


def sig(cols, n_docs, hits, per_segment, deleted=None, masks=None, **body):
    body = dict({"type": "significant_terms", "field": "f"}, **body)
    return R.strip(R.significant(body, cols, n_docs, deleted, masks or {}, hits, per_segment))


def rare(cols, n_docs, hits, per_segment, **body):
    body = dict({"type": "rare_terms", "field": "f"}, **body)
    return R.strip(R.rare(body, cols, n_docs, hits, per_segment))


def test_set_is_picked_by_count_and_ordered_by_score():
    # one segment of 10 docs: a on 6 docs, b on 3, c on 1, one without a value.  The query collects docs 0 .. 4
    docs = [["a"], ["a"], ["a"], ["b"], ["b", "c"], ["a"], ["a"], ["a"], ["b"], []]
    cols, n_docs = world(docs)
    hits = [(0, d) for d in range(5)]
    for mode in (True, False):
        got = sig(cols, n_docs, hits, mode, size=2)
        # foreground: a 3, b 2, c 1 over doc_count 5; background: a 6, b 3, c 1 over bg_count 10 (doc 9 has no value
        # and counts).  size 2 keeps a and b BY COUNT; c, whose score (1/5)/(1/10) = 2.0 is the highest, is cut.
        # scores: a (3/5)/(6/10) = 1.0, b (2/5)/(3/10) = 1.333..: b comes first
        assert [b["key"] for b in got["buckets"]] == ["b", "a"]
        assert got["buckets"][0] == {"key": "b", "doc_count": 2, "bg_count": 3, "score": (2 / 5) / (3 / 10)}
        assert got["buckets"][1] == {"key": "a", "doc_count": 3, "bg_count": 6, "score": (3 / 5) / (6 / 10)}
        assert got["doc_count"] == 5 and got["bg_count"] == 10
        # with room for all three, c leads
        assert [b["key"] for b in sig(cols, n_docs, hits, mode, size=3)["buckets"]] == ["c", "b", "a"]


def test_bg_count_sums_the_segments_whose_foreground_holds_the_key():
    # x is in both segments' background (2 docs and 3 docs); the query collects it in both.  y is in both backgrounds
    # too (1 doc and 2 docs) but the query collects it in segment 1 only: its bg_count is 2, not 3
    s0 = [["x"], ["x"], ["y"], ["z"]]
    s1 = [["x"], ["x"], ["x"], ["y"], ["y"]]
    cols, n_docs = world(s0, s1)
    hits = [(0, 0), (1, 0), (1, 3)]
    for mode in (True, False):
        got = sig(cols, n_docs, hits, mode, size=10)
        by = {b["key"]: b for b in got["buckets"]}
        assert by["x"]["doc_count"] == 2 and by["x"]["bg_count"] == 2 + 3
        assert by["y"]["doc_count"] == 1 and by["y"]["bg_count"] == 2
        assert got["doc_count"] == 3 and got["bg_count"] == 9
        assert by["x"]["score"] == (2 / 3) / (5 / 9) and by["y"]["score"] == (1 / 3) / (2 / 9)
        assert [b["key"] for b in got["buckets"]] == ["y", "x"]  # 1.5 before 1.2


def test_a_segment_without_a_match_still_adds_its_bg_total():
    cols, n_docs = world([["a"], ["b"]], [["a"], ["a"], ["a"]])
    for mode in (True, False):
        got = sig(cols, n_docs, [(0, 0)], mode, size=5)
        assert got["bg_count"] == 5 and got["doc_count"] == 1
        assert got["buckets"] == [{"key": "a", "doc_count": 1, "bg_count": 1, "score": (1 / 1) / (1 / 5)}]


def test_score_is_zero_when_the_filter_removes_every_doc_with_the_key():
    cols, n_docs = world([["a"], ["a"], ["b"], ["b"]])
    masks = {"m": [[False, False, True, True]]}
    for mode in (True, False):
        got = sig(cols, n_docs, [(0, 0), (0, 2)], mode, masks=masks, size=5, background_filter={"name": "m"})
        by = {b["key"]: b for b in got["buckets"]}
        assert got["bg_count"] == 2
        assert by["a"] == {"key": "a", "doc_count": 1, "bg_count": 0, "score": 0.0}
        assert by["b"]["bg_count"] == 2 and by["b"]["score"] == (1 / 2) / (2 / 2)
        # a filter that leaves nothing: bg_count 0, every score 0.0, the order falls back to (count desc, key asc)
        none = sig(cols, n_docs, [(0, 0), (0, 2)], mode, masks={"m": [[False] * 4]}, size=5, background_filter={"name": "m"})
        assert none["bg_count"] == 0 and [(b["key"], b["score"]) for b in none["buckets"]] == [("a", 0.0), ("b", 0.0)]


def test_a_value_twice_and_a_doc_without_a_value():
    cols, n_docs = world([["a", "a"], [], ["a", "b", "a"]])
    for mode in (True, False):
        got = sig(cols, n_docs, all_docs(n_docs), mode, size=5)
        by = {b["key"]: b for b in got["buckets"]}
        assert by["a"]["doc_count"] == 2 and by["a"]["bg_count"] == 2 and by["b"]["doc_count"] == 1
        assert got["doc_count"] == 2  # (doc 1 has no value: not collected ...)
        assert got["bg_count"] == 3   # (... but a live doc of the background)
        r = rare(cols, n_docs, all_docs(n_docs), mode, size=5, max_doc_count=2)
        assert [(b["key"], b["doc_count"]) for b in r["buckets"]] == [("b", 1), ("a", 2)]


def test_deleted_docs_are_not_in_the_background():
    cols, n_docs = world([["a"], ["a"], ["a"], ["b"]])
    got = sig(cols, n_docs, [(0, 0)], False, deleted=[{1, 3}], size=5)
    assert got["bg_count"] == 2 and got["buckets"][0]["bg_count"] == 2


def test_min_doc_count_and_the_tie_orders():
    cols, n_docs = world([["b"], ["b"], ["a"], ["a"], ["c"], ["é"], ["é"]])
    hits = all_docs(n_docs)
    for mode in (True, False):
        got = sig(cols, n_docs, hits, mode, size=10, min_doc_count=2)
        # every score is (n/7)/(n/7) = 1.0: ties fall to count desc, then key bytes asc (é is 0xC3 0xA9: behind b)
        assert [b["key"] for b in got["buckets"]] == ["a", "b", "é"]
        assert [b["key"] for b in sig(cols, n_docs, hits, mode, size=10, min_doc_count=0)["buckets"]] == ["a", "b", "é", "c"]
        assert [b["key"] for b in sig(cols, n_docs, hits, mode, size=10, min_doc_count=3)["buckets"]] == []


def test_rare_max_doc_count_edge():
    cols, n_docs = world([["a"], ["a"], ["a"], ["b"], ["b"], ["c"], ["d"]])
    hits = all_docs(n_docs)
    for mode in (True, False):
        assert [b["key"] for b in rare(cols, n_docs, hits, mode, size=10)["buckets"]] == ["c", "d"]  # default 1
        got = rare(cols, n_docs, hits, mode, size=10, max_doc_count=2)
        assert [(b["key"], b["doc_count"]) for b in got["buckets"]] == [("c", 1), ("d", 1), ("b", 2)]  # 2 is within, 3 is not
        assert [b["key"] for b in rare(cols, n_docs, hits, mode, size=1, max_doc_count=3)["buckets"]] == ["c"]


def test_a_world_where_the_two_modes_differ():
    # rare: k is once in each of two segments.  Per segment it is rare (count 1) in both, the merge sums 2 and the
    # retain drops it; z stays.  All-segment counting sees 2 at once: the same.  With max_doc_count 1 the modes agree
    # here; they differ when a key is beyond the bound in ONE segment and within it in no sum: p has 2 docs in
    # segment 0 (dropped there) and 1 in segment 1 (kept): the reference returns p with 1, the device sees 3
    cols, n_docs = world([["p"], ["p"], ["z"]], [["p"]])
    hits = all_docs(n_docs)
    assert [(b["key"], b["doc_count"]) for b in rare(cols, n_docs, hits, True, size=5)["buckets"]] == [("p", 1), ("z", 1)]
    assert [(b["key"], b["doc_count"]) for b in rare(cols, n_docs, hits, False, size=5)["buckets"]] == [("z", 1)]
    # significant: size 1 truncates every segment to its top key: a (2 docs) in segment 0, b (2 docs) in segment 1;
    # b's doc in segment 0 and its background there are lost.  All-segment counting keeps b with 3 docs
    cols, n_docs = world([["a"], ["a"], ["b"]], [["b"], ["b"], ["c"]])
    hits = all_docs(n_docs)
    ref = sig(cols, n_docs, hits, True, size=1)
    dev = sig(cols, n_docs, hits, False, size=1)
    assert [(b["key"], b["doc_count"], b["bg_count"]) for b in ref["buckets"]] == [("a", 2, 2)]
    assert [(b["key"], b["doc_count"], b["bg_count"]) for b in dev["buckets"]] == [("b", 3, 3)]


def test_a_world_where_the_two_modes_provably_agree():
    # min_doc_count <= 1 and size >= every segment's bucket count: no segment drops or truncates anything, and the
    # merge adds exactly what all-segment counting adds
    cols, n_docs = world([["a"], ["a", "b"], ["c"], []], [["b"], ["b", "c"], ["d"]], [["a"], ["d", "d"]])
    hits = [(0, 0), (0, 1), (1, 1), (1, 2), (2, 1)]
    a, b = sig(cols, n_docs, hits, True, size=4), sig(cols, n_docs, hits, False, size=4)
    assert a == b and len(a["buckets"]) == 4
    # one segment: the two modes are the same computation
    for size in (1, 2, 5):
        assert sig(cols, n_docs[:1], hits[:2], True, size=size) == sig(cols, n_docs[:1], hits[:2], False, size=size)
        assert rare(cols, n_docs[:1], hits[:2], True, size=size) == rare(cols, n_docs[:1], hits[:2], False, size=size)


def test_score_bits():
    assert R.score_bits(0.0) == 0 and R.score_bits(1.0) == 0x3FF0000000000000
