"""tests/request_ref.py against hand-derived tables, one per pair of kinds tests/test_gpu_request.py runs on the
device, and the preconditions of that test's world (tests/request_world.py), all on the CPU.

The hand world: one segment of 12 docs of three tokens each, [0, x, y] with x, y in {1, 2, 3}; doc 6 is tombstoned.
The scored query is term 0 alone: every doc holds it once and all docs are equally long, so every first-pass score is
the same number s0 = 1.0 (the query's weight: every length norm is 1) and score order is (segment, doc) order until
a score stage rewrites the scores.

  term 1: 0 1 3 6 8 10 11      term 2: 0 2 4 6 7 9 10      term 3: 1 2 5 7 8 9 11
  phrase "0 1" (slop 0): docs whose second token is 1: 0 1 3 6 8
  bool  MUST 1, MUST_NOT 3 keeps 0 3 6 10 (scored_docs 4: the tombstoned doc 6 is counted); matched 0 3 10
  val = doc (i64), tag = "a" on even docs and "b" on odd ones, grp = doc % 3, filter F = docs 0 1 2 3
  function_score: (weight 3.0 + 0.5 * val), both under F, REPLACES the score; min_score 2.0 drops every doc outside F
  (its score stays s0): survivors 0 1 2 3 with 3.0 3.5 4.0 4.5."""
import numpy as np
import pytest

from tests import request_ref as R
from tests import request_world as RW
from tests.phrase_ref import segment_from_tokens

F32 = np.float32
MUST, SHOULD, MUST_NOT = 0, 1, 2
DOCS = [[0, 1, 2], [0, 1, 3], [0, 2, 3], [0, 1, 1], [0, 2, 2], [0, 3, 3], [0, 1, 2], [0, 2, 3], [0, 1, 3], [0, 3, 2],
        [0, 2, 1], [0, 3, 1]]
FLT = 0
VAL, TAG, GRP = 0, 1, 2


@pytest.fixture(scope="module")
def H(oracle):
    from searchlite_amd import aggs as A
    from searchlite_amd.script import compile_script
    from tests import bool_ref, fscore_ref, phrase_ref
    seg = segment_from_tokens(DOCS, 4, k1=0.9, b=0.4)
    dead = np.zeros(12, bool)
    dead[6] = True
    seg.deleted, seg.docs = np.packbits(dead, bitorder="little"), 11.0
    segs = [seg]
    qs = RW.csr([[(0, 1.0)]], 1)
    val = [[[d] for d in range(12)]]
    cols = {"val": val, "tag": [[["a"] if d % 2 == 0 else ["b"] for d in range(12)]]}
    flt = [np.arange(12) < 4]
    fcols = fscore_ref.Columns(segs, {VAL: (val, np.dtype(np.int64))}, {FLT: flt})
    h = dict(segs=segs, qs=qs, cols=cols, fcols=fcols, masks={"F": flt}, keys_of={"tag": ["a", "b"]},
             fields={"val": (val, False)}, grp=[[[d % 3] for d in range(12)]],
             agg_fields={"tag": {"id": TAG, "keys": ["a", "b"]}, "val": {"id": VAL}})
    h["cands"] = fscore_ref.all_candidates(oracle, segs, *qs)
    h["s0"] = F32(h["cands"][2][0, 0])
    h["bool"] = ("bool", bool_ref.clauses_of([([(MUST, [1]), (MUST_NOT, [3])], 0)], 1))
    h["tree"] = ("bool_tree", [{"bool": {"must": [{"term": [1]}], "must_not": [{"term": [3]}]}}])
    h["phrase"] = ("phrase", phrase_ref.phrases_of([([(MUST, 0, [[0, 1]])], 0)], 1), None)
    h["fscore"] = [dict(functions=[dict(kind="weight", weight=3.0, filter=FLT),
                                   dict(kind="field_value_factor", field=VAL, factor=0.5, filter=FLT)],
                        score_mode="sum", boost_mode="replace", min_score=2.0)]
    h["script"] = lambda text: [dict(program=compile_script(text, None, {"val": VAL}), boost=1.0)]
    h["plan"] = lambda request: A.agg_spec(request, h["agg_fields"])
    return h


def run(H, clause=None, fscore=None, script=None, order="outer"):
    return R.matched_sets(H["cands"], H["segs"], 1, clause, R.chains_of(1, fscore, script, order), H["fcols"])


def docs(rows):
    return [d for _, d, _ in rows]


def bits(xs):
    return np.asarray(xs, F32).view(np.uint32).tolist()


def test_the_candidates_are_every_doc_of_the_list_with_one_score(H):
    doc, seg, score, count = H["cands"]
    assert int(count[0]) == 12 and sorted(doc[0].tolist()) == list(range(12))  # the tombstoned doc included
    assert len(set(bits(score[0]))) == 1 and float(H["s0"]) == 1.0


@pytest.mark.parametrize("kind", ["bool", "tree"])
def test_clause_then_matched_set(H, kind):
    m = run(H, H[kind])
    assert m["clause_kept"].tolist() == [4] and m["scored"].tolist() == [4] and m["matched"].tolist() == [3]
    assert docs(m["rows"][0]) == [0, 3, 10] and bits([s for _, _, s in m["rows"][0]]) == bits([H["s0"]] * 3)
    none = run(H)
    assert none["scored"].tolist() == [12] and none["matched"].tolist() == [11] and 6 not in docs(none["rows"][0])


def test_phrase_clause(H):
    m = run(H, H["phrase"])
    assert m["scored"].tolist() == [5] and docs(m["rows"][0]) == [0, 1, 3, 8]


def aggs_of(H, m, request):
    plan = H["plan"](request)
    return R.agg_tables(request, plan.nodes, H["cols"], H["masks"], H["keys_of"], m["rows"])


TERMS_STATS = {"t": {"type": "terms", "field": "tag", "aggs": {"s": {"type": "stats", "field": "val"}}}}


def test_bool_x_aggs(H):
    """terms(tag) -> stats(val) over 0 3 10: a = {0, 10}, b = {3}; without the clause a = {0 2 4 8 10}, b = six docs"""
    _, tables, _ = aggs_of(H, run(H, H["bool"]), TERMS_STATS)
    assert tables[0][0, 0].tolist() == [2, 1]
    st = tables[1][0]
    assert [(int(r["count"]), r["min"], r["max"], r["sum"]) for r in st[:, 0]] == [(2, 0.0, 10.0, 10.0), (1, 3.0, 3.0, 3.0)]
    _, plain, _ = aggs_of(H, run(H), TERMS_STATS)
    assert plain[0][0, 0].tolist() == [5, 6]


def test_bool_x_histogram_and_cardinality(H):
    request = {"h": {"type": "histogram", "field": "val", "interval": 5}, "c": {"type": "cardinality", "field": "tag"}}
    _, _, resp = aggs_of(H, run(H, H["bool"]), request)
    assert [(b["key"], b["doc_count"]) for b in resp[0]["h"]["buckets"]] == [(0.0, 2), (10.0, 1)]
    assert resp[0]["c"]["value"] == 2


def test_bool_x_fscore(H):
    """0 3 6 10 enter the score stage: 0 and 3 are under F (3.0 and 4.5); 6 is tombstoned, so the registered bitmap
    gives it no value and it keeps s0; 10 is outside F: both fall below min_score"""
    m = run(H, H["bool"], H["fscore"])
    assert m["clause_kept"].tolist() == [4] and m["scored"].tolist() == [2] and m["matched"].tolist() == [2]
    assert [(d, float(s)) for _, d, s in m["rows"][0]] == [(3, 4.5), (0, 3.0)]


def test_bool_x_script_and_both_orders_with_fscore(H):
    m = run(H, H["bool"], None, H["script"]("_score + val"))
    assert docs(m["rows"][0]) == [10, 3, 0] and m["scored"].tolist() == [4]
    outer = run(H, H["bool"], H["fscore"], H["script"]("_score * 2"), "outer")  # script_score{function_score}
    assert [(d, float(s)) for _, d, s in outer["rows"][0]] == [(3, 9.0), (0, 6.0)]
    inner = run(H, H["bool"], H["fscore"], H["script"]("_score * 2"), "inner")  # function_score{script_score}
    # the script doubles s0 first: docs 6 and 10, outside F, keep 2.0, which is not below min_score
    assert [(d, float(s)) for _, d, s in inner["rows"][0]] == [(3, 4.5), (0, 3.0), (10, 2.0)]
    assert inner["scored"].tolist() == [4] and outer["scored"].tolist() == [2]


@pytest.mark.parametrize("sort", [None, [("val", "desc"), ("_score", "desc")]], ids=["score", "sorted"])
def test_bool_x_cursor_three_pages(H, sort):
    rows = R.ordered(run(H, H["bool"])["rows"], sort, H["fields"])
    want = [0, 3, 10] if sort is None else [10, 3, 0]
    assert docs(rows[0]) == want
    got, after = [], None
    for page in range(3):
        cursors, behind, matched, seen = R.paged(rows, [after], sort, H["fields"])
        assert matched.tolist() == [3 - page] and seen.tolist() == [1]
        assert (cursors[0] is None) == (page == 0)
        if page:
            vals, s, d = cursors[0]
            assert (s, d) == (0, want[page - 1]) and len(vals) == (1 if sort is None else 2)
        arr = R.as_arrays(behind, 1)
        assert arr[3].tolist() == [1]
        got.append(int(arr[0][0, 0]))
        after = page + 1
    assert got == want


def test_bool_x_collapse_and_fscore_x_collapse(H):
    """grp = doc % 3.  Without a clause group 1 is led by doc 1; the clause takes doc 1 away and doc 10 leads it"""
    spec = dict(group_limit=3, inner_from=0, inner_size=2, inner_sort=[("val", "desc")])
    plain = R.collapse_arrays(R.as_arrays(run(H)["rows"], 11), H["grp"], spec, None, H["fields"])
    assert plain["group_doc"][0].tolist() == [0, 1, 2]
    got = R.collapse_arrays(R.as_arrays(run(H, H["bool"])["rows"], 11), H["grp"], spec, None, H["fields"])
    assert got["total_groups"].tolist() == [2] and got["group_doc"][0].tolist() == [0, 10, 0]
    assert got["group_ord"][0].tolist() == [0, 1, 0] and got["group_size"][0].tolist() == [2, 1, 0]
    assert got["inner_count"][0].tolist() == [1, 0, 0] and got["inner_doc"][0, 0].tolist() == [3, 0]
    fs = R.collapse_arrays(R.as_arrays(run(H, None, H["fscore"])["rows"], 11), H["grp"], spec, None, H["fields"])
    # rows 3 (4.5) 2 (4.0) 1 (3.5) 0 (3.0): groups 0, 2, 1 by first appearance; doc 0 is doc 3's member
    assert fs["group_doc"][0].tolist() == [3, 2, 1] and fs["group_ord"][0].tolist() == [0, 2, 1]
    assert fs["group_score"][0].tolist() == [4.5, 4.0, 3.5] and fs["inner_doc"][0, 0].tolist() == [0, 0]


def test_bool_x_rescore(H, oracle):
    """rescore by term 2 over a window of 2: without the clause the window holds docs 0 and 1; with it docs 0 and 3,
    of which only doc 0 holds term 2; doc 10 holds it too but lies outside the window"""
    from tests import rescore_ref
    rs = dict(q_offsets=np.array([0, 1], np.uint32), q_terms=np.array([[2]], np.uint32), q_weights=np.array([1.0], F32),
              window=2)
    maps = rescore_ref.rescore_maps(oracle, H["segs"], rs)
    assert (0, 10) in maps[0] and (0, 3) not in maps[0]
    doc, seg, score, count, first, rsc, flag = R.rescored(R.as_arrays(run(H, H["bool"])["rows"], 3), maps, 2)
    assert doc[0].tolist() == [0, 3, 10] and flag[0].tolist() == [1, 0, 0] and count.tolist() == [3]
    assert bits(first[0]) == bits([H["s0"]] * 3) and bits(score[0, 1:]) == bits([H["s0"]] * 2)
    assert bits(score[0, :1]) == bits([F32(H["s0"] + maps[0][(0, 0)])]) and rsc[0, 0] == maps[0][(0, 0)]


def test_collectors_see_the_rewritten_scores_and_the_matched_set(H):
    """fscore x aggs + top_hits, and bool x {top_hits by _score, composite with one after page, rare_terms}"""
    m = run(H, None, H["fscore"])
    _, tables, _ = aggs_of(H, m, {"t": {"type": "terms", "field": "tag"}})
    assert tables[0][0, 0].tolist() == [2, 2]
    (total, hits), = R.top_hits_root(m["rows"], 2, 0, [("_score", "desc")], H["fields"])
    assert total == 4 and [(d, float(s)) for _, d, s in hits] == [(3, 4.5), (2, 4.0)]
    b = run(H, H["bool"])
    (total, hits), = R.top_hits_root(b["rows"], 2, 0, [("_score", "desc")], H["fields"])
    assert total == 3 and docs(hits) == [0, 3]
    body = {"type": "composite", "size": 1, "sources": [{"type": "terms", "name": "tag", "field": "tag"}]}
    (rows, more), = R.composite_page(body, H["cols"], (), b["rows"])
    assert more and [(k, len(d)) for k, d in rows] == [(("a",), 2)]
    (rows, more), = R.composite_page(body, H["cols"], (), b["rows"], after={"tag": "a"})
    assert not more and [(k, len(d)) for k, d in rows] == [(("b",), 1)]
    rare = {"type": "rare_terms", "field": "tag", "size": 5, "max_doc_count": 1}
    resp, = R.term_bucket_responses(rare, H["cols"], [12], [{6}], H["masks"], b["rows"])
    assert [(x["key"], x["doc_count"]) for x in resp["buckets"]] == [("b", 1)]


def test_chains(H):
    """bool_tree + fscore + sort + aggs + collapse, and phrase + script + cursor + collapse"""
    sort = [("val", "asc"), ("_score", "desc")]
    m = run(H, H["tree"], H["fscore"])
    rows = R.ordered(m["rows"], sort, H["fields"])
    assert [(d, float(s)) for _, d, s in rows[0]] == [(0, 3.0), (3, 4.5)]
    _, tables, _ = aggs_of(H, m, {"t": {"type": "terms", "field": "tag"}})
    assert tables[0][0, 0].tolist() == [1, 1]
    got = R.collapse_arrays(R.as_arrays(rows, 5), H["grp"], dict(group_limit=2, inner_size=1), sort, H["fields"])
    assert got["total_groups"].tolist() == [1] and got["group_doc"][0].tolist() == [0, 0] and got["inner_doc"][0, 0].tolist() == [3]
    p = run(H, H["phrase"], None, H["script"]("_score + val"))
    assert docs(p["rows"][0]) == [8, 3, 1, 0]
    cursors, behind, matched, _ = R.paged(p["rows"], [1])
    assert cursors[0][1:] == (0, 8) and matched.tolist() == [3] and docs(behind[0]) == [3, 1, 0]
    got = R.collapse_arrays(R.as_arrays(behind, 5), H["grp"], dict(group_limit=2, inner_size=1), None, H["fields"])
    assert got["group_doc"][0].tolist() == [3, 1] and got["inner_doc"][0].reshape(-1).tolist() == [0, 0]


# ---- the worlds of the GPU test: what its cases need, per batch and query class ---------------------------------------
@pytest.mark.parametrize("which", ["few", "many"])
def test_world_preconditions(oracle, which):
    from tests import fscore_ref
    w = RW.build(which)
    w["cands"] = fscore_ref.all_candidates(oracle, w["segs"], *w["qs"])
    RW.preconditions(w)
