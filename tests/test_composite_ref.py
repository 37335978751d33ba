"""tests/composite_ref.py against hand-derived answers: the reference's own paging case restated as data, the order
of keys, the two zero buckets, the skip and dedup rules, an ignored `after`."""
import math

from tests import composite_ref as R

TAG = {"type": "terms", "name": "tag", "field": "tag"}
X = {"type": "histogram", "name": "x", "field": "x", "interval": 1.0}


def docs_of(columns):
    return [(s, d) for s, seg in enumerate(next(iter(columns.values()))) for d in range(len(seg))]


def respond(body, columns, f64=("x",)):
    return R.respond(body, columns, set(f64), {}, docs_of(columns))


def test_reference_paging_case():
    # searchlite-core/tests/aggregations.rs, composite_aggregation_paginates: tags a, b, c; size 2
    cols = {"tag": [[["a"], ["b"], ["c"]]]}
    body = {"type": "composite", "sources": [TAG], "size": 2}
    first = respond(body, cols)
    assert [b["key"] for b in first["buckets"]] == [{"tag": "a"}, {"tag": "b"}]
    assert [b["doc_count"] for b in first["buckets"]] == [1, 1]
    assert first["after_key"] == {"tag": "b"}
    second = respond(dict(body, after=first["after_key"]), cols)
    assert [b["key"] for b in second["buckets"]] == [{"tag": "c"}]
    assert "after_key" not in second


def test_key_order_is_utf8_bytes():
    # "Z" < "a" < "ab" < "b" < "é" (0xC3) < "中" (0xE4) < "😀" (0xF0): bytes, not UTF-16 units, a prefix first
    keys = ["é", "b", "😀", "ab", "Z", "中", "a", "￿"]
    cols = {"tag": [[[k] for k in keys]]}
    got = [b["key"]["tag"] for b in respond({"type": "composite", "sources": [TAG], "size": 10}, cols)["buckets"]]
    assert got == ["Z", "a", "ab", "b", "é", "中", "￿", "😀"]  # (U+FFFF is 3 bytes, below any 4-byte character)
    assert got == sorted(keys, key=lambda s: s.encode("utf-8")) and got != sorted(keys, key=lambda s: s.encode("utf-16-be"))


def test_two_zero_buckets():
    cols = {"x": [[[-0.0], [0.0], [0.25], [-0.25], [-1e-320]]]}  # (a negative subnormal floors to -1, not to -0.0)
    got = respond({"type": "composite", "sources": [dict(X, interval=0.5)], "size": 10}, cols)["buckets"]
    keys = [b["key"]["x"] for b in got]
    assert [math.copysign(1.0, k) for k in keys] == [-1.0, -1.0, 1.0] and keys == [-0.5, 0.0, 0.0]
    assert [b["doc_count"] for b in got] == [2, 1, 2]  # -0.25 and -1e-320 | -0.0 | 0.0 and 0.25
    # `after` = -0.0 gives the 0.0 bucket next; `after` = 0.0 passes both
    nxt = respond({"type": "composite", "sources": [dict(X, interval=0.5)], "size": 1, "after": {"x": -0.0}}, cols)
    assert R.f64_order(nxt["buckets"][0]["key"]["x"]) == R.f64_order(0.0) and "after_key" not in nxt
    assert respond({"type": "composite", "sources": [dict(X, interval=0.5)], "size": 1, "after": {"x": 0.0}}, cols)["buckets"] == []


def test_skip_dedup_and_cross_product():
    cols = {"tag": [[["a", "b", "a"], [], ["b"]], [["a"]]],
            "x": [[[0.5, 1.5, 0.7], [2.0], []], [[3.0, 3.5]]]}
    got = respond({"type": "composite", "sources": [TAG, X], "size": 10}, cols)
    # doc (0,0): {a, b} x {0, 1} once each (a twice, 0.5 and 0.7 in one bucket); (0,1) lacks tag; (0,2) lacks x
    assert [(b["key"]["tag"], b["key"]["x"], b["doc_count"]) for b in got["buckets"]] == [
        ("a", 0.0, 1), ("a", 1.0, 1), ("a", 3.0, 1), ("b", 0.0, 1), ("b", 1.0, 1)]
    assert "after_key" not in got
    # an i64 column under a histogram source: every doc is skipped
    assert respond({"type": "composite", "sources": [TAG, X], "size": 10}, cols, f64=())["buckets"] == []


def test_after_filter_and_ignored_after():
    cols = {"tag": [[["a"], ["b"], ["c"], ["b"]]], "x": [[[1.0], [2.0], [3.0], [5.0]]]}
    body = {"type": "composite", "sources": [TAG, X], "size": 2}
    full = respond(dict(body, size=10), cols)["buckets"]
    assert len(full) == 4
    page = respond(dict(body, after={"tag": "b", "x": 2.0}), cols)
    assert [b["key"] for b in page["buckets"]] == [{"tag": "b", "x": 5.0}, {"tag": "c", "x": 3.0}] and "after_key" not in page
    between = respond(dict(body, after={"tag": "b", "x": 2.5}), cols)
    assert [b["key"] for b in between["buckets"]] == [{"tag": "b", "x": 5.0}, {"tag": "c", "x": 3.0}]
    absent = respond(dict(body, after={"tag": "aa", "x": 99.0}), cols)
    assert [b["key"] for b in absent["buckets"]] == [{"tag": "b", "x": 2.0}, {"tag": "b", "x": 5.0}]
    assert absent["after_key"] == {"tag": "b", "x": 5.0}
    # ignored: a missing name, a terms part that is no string, a histogram part that is no number
    for bad in ({"tag": "b"}, {"tag": 7, "x": 2.0}, {"tag": "b", "x": "2"}, {"tag": "b", "x": True}, {"tag": "b", "x": None}):
        got = respond(dict(body, after=bad), cols)
        assert [b["key"] for b in got["buckets"]] == [{"tag": "a", "x": 1.0}, {"tag": "b", "x": 2.0}], bad
        assert got["after_key"] == {"tag": "b", "x": 2.0}


def test_children_collect_once_per_tuple():
    cols = {"tag": [[["a", "b"], ["a"]]], "x": [[[1.0, 2.0], [4.0]]]}
    body = {"type": "composite", "sources": [TAG], "size": 5, "aggs": {"s": {"type": "stats", "field": "x"}}}
    got = respond(body, cols)["buckets"]
    assert [(b["key"]["tag"], b["doc_count"], b["aggregations"]["s"]["count"], b["aggregations"]["s"]["sum"])
            for b in got] == [("a", 2, 3, 7.0), ("b", 1, 2, 3.0)]
