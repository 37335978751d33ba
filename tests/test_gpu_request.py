"""Compound requests on the device (slg_batch_prepare_request) through the C ABI against tests/request_ref.py.

Tolerance 0: docs, segments, scores (bit patterns), counts, matched counts, scored_docs, aggregation tables (the
columns hold exactly summable values, so the sums too: inside the bound of tests/test_gpu_aggs.py), top_hits lists,
composite pages, term buckets, collapse groups and inner hits, rescore details; rows past a count are zero.  The rows
of a request with collectors or collapse equal those of the same request without them, bit for bit.

The worlds and what they must provide: tests/request_world.py.  The scoring kernel is chosen per batch, so the 12
three-term queries (fixture W: the few-term kernel) and the 12-list query (fixture M: the many-term kernel) are two
batches over the same segments; the pairs, chains, k edges, two runs and the identity with the legacy batches run on
both (fixture B).  RW.preconditions() asserts, on the CPU and before an index is opened, what the cases are about
(tests/test_request_ref.py runs it without a device too)."""
import copy

import numpy as np
import pytest

from tests import collapse_ref, composite_ref, request_ref as R, request_world as RW, term_buckets_ref
from tests.test_gpu_bool import same

pytestmark = pytest.mark.gpu
F32 = np.float32
KINDS = RW.KINDS
AGGS = {"t": {"type": "terms", "field": "tag", "aggs": {"s": {"type": "stats", "field": "frac"}}},
        "h": {"type": "histogram", "field": "num", "interval": 7, "offset": 0.25},
        "c": {"type": "cardinality", "field": "tag"}}
COLLAPSE = dict(group_limit=5, inner_from=0, inner_size=3, inner_sort=[("low", "desc"), ("_score", "desc")])


matched, preconditions = RW.matched, RW.preconditions


def register(w, ix):
    """the world's columns and filters onto an index, in the order tests/request_world.py fixes their ids by"""
    from searchlite_amd import aggs as A, filters as F
    for s, seg in enumerate(w["segs"]):
        ix.set_positions(s, seg.pos_offsets, seg.positions)
    fields = {}
    for name in ("tag", "grp"):
        keys = w["keys_of"][name]
        ord_of = {k: i for i, k in enumerate(keys)}
        ords = [[np.array([ord_of[v] for v in d], np.uint32) for d in col] for col in w["cols"][name]]
        fields[name] = {"id": ix.add_agg_keyword_field(ords, len(keys)), "keys": keys}
    fields["num"] = {"id": ix.add_agg_field(w["cols"]["num"], np.int64)}
    fields["frac"] = {"id": ix.add_agg_field(w["cols"]["frac"], np.float64)}
    assert {n: f["id"] for n, f in fields.items()} == RW.FIELD
    fields["low"] = {"sort_id": ix.add_sort_field(w["low"], np.int64)}
    assert fields["low"]["sort_id"] == RW.SORT_FIELD["low"]
    assert ix.add_filter(w["masks"]["half"]) == RW.FILTER["half"]
    tree = F.compile_filter({"KeywordIn": {"field": "tag", "values": RW.TREE_VALUES}},
                            {"tag": {"id": fields["tag"]["id"], "kind": "keyword", "keys": RW.TAG_KEYS}})
    assert ix.add_filter_trees([tree])[0] == RW.FILTER["tree"]
    fields[A.FILTERS] = lambda body: RW.FILTER[body["name"]]
    return fields


def open_world(oracle, which):
    import searchlite_amd as sa
    from tests import fscore_ref
    w = RW.build(which)
    w["oracle"] = oracle
    w["cands"] = fscore_ref.all_candidates(oracle, w["segs"], *w["qs"])
    preconditions(w)  # (on the CPU, before the device runs)
    w["ix"] = ix = sa.GpuIndex(w["segs"])
    # the batch's scoring kernel, from the plan facts: the few-term kernel takes a batch whose longest query has at
    # most uniform_max_terms lists, every other batch runs on the many-term kernel
    assert (w["max_lists"] <= int(ix.tuning().uniform_max_terms)) == (which == "few")
    w["agg_fields"] = register(w, ix)
    # the registered tree's bitmap is the mask the reference uses
    for got, mask, seg in zip(ix.fetch_filter(RW.FILTER["tree"]), w["leaf_masks"][RW.FILTER["tree"]], w["segs"]):
        assert np.array_equal(np.asarray(got, bool)[:seg.n_docs], mask), "the tree filter's bitmap"
    return w


@pytest.fixture(scope="module")
def W(oracle):
    """the 12 three-term queries: the few-term kernel"""
    w = open_world(oracle, "few")
    yield w
    w["ix"].close()


@pytest.fixture(scope="module")
def M(oracle):
    """the 12-list query: the many-term kernel"""
    w = open_world(oracle, "many")
    yield w
    w["ix"].close()


@pytest.fixture(params=["few", "many"])
def B(request, W, M):
    return W if request.param == "few" else M


def ids_of(sort):
    return None if sort is None else [(p if p == "_score" else RW.SORT_FIELD[p], o) for p, o in sort]


def stage_args(w, clause, fscore, script, order):
    kw = {} if clause is None else dict(RW.clause_of(w, clause)[1])
    if fscore:
        kw["fscore"] = w["fscore"]
    if script:
        kw.update(script=RW.scripts_of(w), script_order=order)
    return kw


def plan_of(w, aggs, extra):
    from searchlite_amd import aggs as A
    if aggs is None and extra is None:
        return None
    return A.agg_spec(dict(aggs or {}, **(extra or {})), w["agg_fields"])


def same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def check_aggs(w, plan, aggs, rows, tables, layout, what):
    from searchlite_amd import aggs as A
    want_layout, want_tables, want_resp = R.agg_tables(aggs, plan.nodes, w["cols"], w["masks"], w["keys_of"], rows)
    for i, (g, wt) in enumerate(zip(tables, want_tables)):
        gl, wl = layout[i], want_layout[i]
        assert (gl["parent_rows"], gl["rows"], gl["first_id"]) == (wl["parent_rows"], wl["rows"], wl["first_id"]), \
            f"{what} node {i}: layout {gl} != {wl}"
        assert g.shape == wt.shape, f"{what} node {i}: shape"
        if gl["is_stats"]:
            for f in ("count", "min", "max", "sum"):  # (exactly summable values: the sums are equal, not just within the bound)
                assert np.array_equal(g[f], wt[f]), f"{what} node {i}: stats {f} differ"
        else:
            assert np.array_equal(g, wt), f"{what} node {i}: cells differ at {np.argwhere(g != wt)[:5].tolist()}"
    for q in range(w["nq"]):
        assert A.shape(plan, layout, tables, q) == want_resp[q], f"{what}: response of query {q}"


def check(w, what, clause=None, fscore=False, script=False, order="outer", sort=None, after=None, k=11, aggs=None,
          extra=None, collapse=None, rescore=None, q_filter=None, runs=1, composite_after=None):
    """one compound request against request_ref, and against the same request without collectors / collapse
    -> dict(page = the expected rows, m = the matched sets, got = the fetched rows)"""
    from searchlite_amd import aggs as A
    ix, qs = w["ix"], w["qs"]
    m = matched(w, clause, fscore, script, order, q_filter)
    rows = R.ordered(m["rows"], sort, w["fields"])
    want_matched, cursors = m["matched"], None
    if after is not None:
        cursors, rows, want_matched, want_seen = R.paged(rows, after, sort, w["fields"])
    page = R.as_arrays(rows, k)
    plan = plan_of(w, aggs, extra)
    kw = dict(stage_args(w, clause, fscore, script, order), sort=ids_of(sort), cursors=cursors, q_filter=q_filter)
    full = dict(kw)
    if plan is not None:
        full["aggs"] = plan
    if collapse is not None:
        full["collapse"] = dict(collapse, field=RW.FIELD["grp"], inner_sort=ids_of(collapse.get("inner_sort")))
    if rescore is not None:
        full["rescore"] = rescore
    with ix.prepare_request(*qs, k, **full) as b:
        if composite_after is not None:
            b.set_composite_after([A.composite_lower_bound(b.composite_layout(), plan, a) for a in composite_after])
        for run in range(runs):
            b.run()
            got = b.fetch(want_stats=True)
            at = f"{what} run {run}"
            if rescore is None:
                same(got[:4], page, at)
            else:
                maps = w.setdefault("_rs_maps", {}).get(id(rescore))
                if maps is None:
                    from tests import rescore_ref
                    maps = w["_rs_maps"][id(rescore)] = rescore_ref.rescore_maps(w["oracle"], w["segs"], rescore)
                want_rs = R.rescored(page, maps, rescore["window"], rescore.get("mode"))
                same(got[:4], want_rs[:4], at + " rescored rows")
                for g, wt, name in zip(b.rescore_details(), want_rs[4:], ("first_score", "rescore_score", "rescored")):
                    same_bytes(g, wt, f"{at}: {name}")
            sd = [int(got[4][q].scored_docs) for q in range(w["nq"])]
            assert sd == m["scored"].tolist(), f"{at}: scored_docs {sd} != {m['scored'].tolist()}"
            if sort is not None or after is not None or plan is not None:
                assert b.matched_counts().tolist() == want_matched.tolist(), f"{at}: matched counts"
            if after is not None:
                assert b.cursor_seen().tolist() == want_seen.tolist(), f"{at}: cursor_seen"
            if aggs is not None:
                check_aggs(w, plan, aggs, m["rows"], b.aggs(), b.agg_layout(), at)
            if plan is not None and plan.top_hits_nodes:
                th = b.top_hits()
                (name, body), = extra.items()
                assert not th["status"].any(), at
                tsort = [(p["field"], p["order"]) for p in body.get("sort", [])]
                for q, (total, hits) in enumerate(R.top_hits_root(rows, body["size"], body.get("from", 0), tsort, w["fields"])):
                    n = int(th["nodes"][0]["count"][q, 0])
                    have = [(int(th["nodes"][0]["seg"][q, 0, i]), int(th["nodes"][0]["doc"][q, 0, i])) for i in range(n)]
                    assert have == [(s, d) for s, d, _ in hits], f"{at}: top_hits of query {q}"
                    assert th["nodes"][0]["score"][q, 0, :n].view(np.uint32).tolist() == \
                        np.asarray([sc for _, _, sc in hits], F32).view(np.uint32).tolist(), f"{at}: top_hits scores of query {q}"
                    assert total == int(want_matched[q])
                    assert not th["nodes"][0]["doc"][q, 0, n:].any() and not th["nodes"][0]["score"][q, 0, n:].any()
            if plan is not None and plan.composite is not None:
                from tests.test_gpu_composite import assert_same_response
                (name, body), = extra.items()
                lay, pg = b.composite_layout(), b.composite()
                for q, d in enumerate(R.docs_of(m["rows"])):
                    buckets = composite_ref.collect(body["sources"], w["cols"], ("frac",), d)
                    brows, more = composite_ref.finalize(body["sources"], buckets, body["size"],
                                                         None if composite_after is None else composite_after[q])
                    want = {"type": "composite", "buckets": [{"key": {s["name"]: p for s, p in zip(body["sources"], key)},
                                                              "doc_count": len(docs)} for key, docs in brows]}
                    if more and brows:
                        want["after_key"] = want["buckets"][-1]["key"]
                    assert_same_response(A.shape_composite(plan, lay, pg, q), want, f"{at}: composite of query {q}")
            if plan is not None and plan.term_buckets is not None:
                lay, tb = b.term_buckets_layout(), b.term_buckets()
                dead = [set(np.nonzero(~RW.alive(s))[0].tolist()) for s in w["segs"]]
                for name, body in extra.items():
                    resp = R.term_bucket_responses(body, w["cols"], w["n_docs"], dead, w["masks"], m["rows"])
                    for q in range(w["nq"]):
                        assert A.shape_term_buckets(plan, lay, tb, q)[name] == term_buckets_ref.strip(resp[q]), \
                            f"{at}: {name} of query {q}"
            if collapse is not None:
                want = R.collapse_arrays(page, w["grp_column"], collapse, sort, w["fields"])
                collapse_ref.assert_same_arrays(b.collapse_groups(), want, at)
    if plan is not None or collapse is not None:  # the same request without collectors / collapse: the rows, bit for bit
        with ix.prepare_request(*qs, k, **kw) as base:
            base.run()
            same(base.fetch()[:4], got[:4], what + " vs the request without collectors / collapse")
    return dict(page=page, m=m, got=got)


# ---- identity: one kind through the new entry is the legacy batch ------------------------------------------------------
def fetched(b, w):
    """everything a batch gives, as bytes"""
    b.run()
    out = [np.ascontiguousarray(a).tobytes() for a in b.fetch()[:4]]
    blk, n = b.device_result_block()
    out.append(int(n))
    if b.sorted or b.after or b.agg_spec is not None or b.top_hits_spec is not None or b.composite_spec is not None \
            or b.term_bucket_spec is not None:
        out.append(b.matched_counts().tobytes())
    if b.after:
        out.append(b.cursor_seen().tobytes())
    if b.agg_spec is not None:
        out += [t.tobytes() for t in b.aggs()]
    if b.top_hits_spec is not None:
        th = b.top_hits()
        out += [th["status"].tobytes()] + [x[n_].tobytes() for x in th["nodes"] for n_ in ("doc", "seg", "score", "count")]
    if b.composite_spec is not None:
        pg = b.composite()
        out += [pg[n_].tobytes() for n_ in ("keys", "n_buckets", "has_more", "counts")]
    if b.term_bucket_spec is not None:
        for nd in b.term_buckets()["nodes"]:
            out += [nd[n_].tobytes() for n_ in ("ords", "doc_counts", "bg_counts", "score_bits", "n_buckets")]
    if b.is_rescore:
        out += [x.tobytes() for x in b.rescore_details()]
    if b.is_collapse:
        out += [v.tobytes() for _, v in sorted(b.collapse_groups().items())]
    return out


def legacy_kinds(w):
    from tests.test_gpu_composite import cmp
    rs = rescore_of(w)
    cur = R.paged(R.ordered(matched(w)["rows"]), [3] * w["nq"])[0]
    col = dict(COLLAPSE, field=RW.FIELD["grp"], inner_sort=ids_of(COLLAPSE["inner_sort"]))
    return {
        "plain": {}, "sorted": dict(sort=ids_of(RW.SORT2)), "after": dict(cursors=cur),
        "bool": RW.clause_of(w, "bool")[1], "phrase": RW.clause_of(w, "phrase")[1], "bool_tree": RW.clause_of(w, "bool_tree")[1],
        "fscore": dict(fscore=w["fscore"]), "script": dict(script=RW.scripts_of(w)),
        "script+fscore": dict(script=RW.scripts_of(w), fscore=w["fscore"], script_order="inner"),
        "aggs": dict(aggs=plan_of(w, AGGS, None)), "top_hits": dict(aggs=plan_of(w, AGGS, TOP_HITS)),
        "composite": dict(aggs=plan_of(w, None, {"cp": cmp([{"type": "terms", "name": "tag", "field": "tag"}], 3)})),
        "term_buckets": dict(aggs=plan_of(w, None, SIG)), "rescore": dict(rescore=rs),
        "collapse": dict(collapse=col, sort=ids_of(RW.SORT2)),
    }


TOP_HITS = {"best": {"type": "top_hits", "size": 3, "sort": [{"field": "_score", "order": "desc"}]}}
SIG = {"sig": {"type": "significant_terms", "field": "tag", "size": 4}, "rare": {"type": "rare_terms", "field": "grp", "size": 3,
                                                                               "max_doc_count": 100}}


def rescore_of(w):
    """rescore by term 2 (and 5), window RW.RESCORE_WINDOW = 7: with 11 rows the window ends inside the rows"""
    if "_rescore" not in w:
        offs, terms, ws = RW.csr([[(2, 1.0), (5, 0.5)]] * w["nq"], w["n_segs"])
        w["_rescore"] = dict(q_offsets=offs, q_terms=terms, q_weights=ws, window=RW.RESCORE_WINDOW, mode=0)
    return w["_rescore"]


def test_one_kind_through_the_request_is_the_legacy_batch(B):
    W = B
    for name, kw in legacy_kinds(W).items():
        with W["ix"].prepare(*W["qs"], 11, **kw) as old, W["ix"].prepare_request(*W["qs"], 11, **kw) as new:
            a, b = fetched(old, W), fetched(new, W)
            assert len(a) == len(b) and all(x == y for x, y in zip(a, b)), f"{name}: the request's batch differs from the legacy one"


# ---- pairs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", [None, RW.SORT2], ids=["score", "sorted"])
@pytest.mark.parametrize("clause", KINDS)
def test_clause_x_aggs(B, clause, sort):
    W = B
    check(W, f"{clause} x aggs", clause=clause, sort=sort, aggs=AGGS)


def test_bool_x_top_hits_composite_term_buckets(B):
    W = B
    from tests.test_gpu_composite import cmp
    check(W, "bool x top_hits", clause="bool", extra=TOP_HITS)
    body = cmp([{"type": "terms", "name": "tag", "field": "tag"}, {"type": "histogram", "name": "frac", "field": "frac", "interval": 8.0}], 4)
    out = check(W, "bool x composite", clause="bool", extra={"cp": body})
    # one `after` page: behind the first page's last key of every query that has more
    afters = []
    for d in R.docs_of(out["m"]["rows"]):
        rows, more = composite_ref.finalize(body["sources"], composite_ref.collect(body["sources"], W["cols"], ("frac",), d), 4, None)
        afters.append({s["name"]: p for s, p in zip(body["sources"], rows[-1][0])} if more else None)
    assert sum(a is not None for a in afters) >= (8 if W["which"] == "few" else 1)
    check(W, "bool x composite after", clause="bool", extra={"cp": body}, composite_after=afters)
    check(W, "bool x term_buckets", clause="bool", extra=SIG)


def test_bool_x_fscore_and_script(B):
    W = B
    out = check(W, "bool x fscore", clause="bool", fscore=True, k=257)
    b = matched(W, "bool")
    assert (out["m"]["scored"] < b["clause_kept"])[[0, 1, 2] if W["which"] == "few" else [0]].all()
    check(W, "bool x script", clause="bool", script=True)
    outer = check(W, "bool x fscore x script outer", clause="bool", fscore=True, script=True, order="outer")
    inner = check(W, "bool x fscore x script inner", clause="bool", fscore=True, script=True, order="inner")
    assert not np.array_equal(outer["page"][2], inner["page"][2])
    check(W, "bool x fscore sorted", clause="bool", fscore=True, sort=RW.SORT2)


@pytest.mark.parametrize("sort", [None, RW.SORT2], ids=["score", "sorted"])
def test_bool_x_cursor_three_pages(B, sort):
    W = w = B
    few = w["which"] == "few"
    k, after, pages = 11, [None] * w["nq"], []
    for p in range(3):
        out = check(W, f"bool x cursor page {p}", clause="bool", sort=sort, after=after, k=k)
        pages.append(out["got"])
        after = [(p + 1) * k if int(out["m"]["matched"][q]) > (p + 1) * k else None for q in range(w["nq"])]
        assert sum(a is not None for a in after) >= (10 if few else 1)
    one = check(W, "bool one page of 3k", clause="bool", sort=sort, k=3 * k)["got"]
    for q in range(w["nq"]):
        if int(one[3][q]) < 3 * k:
            continue
        for i in range(3):
            cat = np.concatenate([pg[i][q, :k] for pg in pages])
            assert np.array_equal(cat.view(np.uint32), one[i][q].view(np.uint32)), f"query {q}: three pages are one page of 3k"


def test_collapse_behind_clause_and_score_stages(B):
    W = B
    check(W, "bool x collapse", clause="bool", collapse=COLLAPSE, k=65)
    check(W, "fscore x collapse", fscore=True, collapse=COLLAPSE, k=65)
    check(W, "bool x collapse x cursor", clause="bool", collapse=COLLAPSE, after=[5] * 6 + [None] + [5] * 5 if W["which"] == "few" else [5], k=33)


def test_bool_x_rescore(B):
    W = B
    """window 7: without the clause other docs hold ranks 0 .. 6 (RW.preconditions asserts it for RW.CROSSING and the
    12-list query), so the window crosses the former ranks of clause-rejected docs"""
    check(W, "bool x rescore", clause="bool", rescore=rescore_of(W))


def test_fscore_x_aggs_and_top_hits(B):
    W = B
    check(W, "fscore x aggs + top_hits", fscore=True, aggs=AGGS, extra=TOP_HITS)


def test_search_request_returns_what_was_asked_for(B):
    W = B
    """GpuIndex.search_request: prepare_request, one run and the results of every kind asked for, by name"""
    kw = dict(stage_args(W, "bool", True, False, "outer"), aggs=plan_of(W, AGGS, TOP_HITS), sort=ids_of(RW.SORT2),
              collapse=dict(COLLAPSE, field=RW.FIELD["grp"], inner_sort=ids_of(COLLAPSE["inner_sort"])))
    out = W["ix"].search_request(*W["qs"], 11, want_stats=True, **kw)
    assert sorted(out) == sorted(["doc", "seg", "score", "count", "stats", "matched", "aggs", "agg_layout", "top_hits", "collapse"])
    m = matched(W, "bool", fscore=True)
    page = R.as_arrays(R.ordered(m["rows"], RW.SORT2, W["fields"]), 11)
    same((out["doc"], out["seg"], out["score"], out["count"]), page, "search_request")
    assert out["matched"].tolist() == m["matched"].tolist()
    assert [int(s.scored_docs) for s in out["stats"]] == m["scored"].tolist()
    check_aggs(W, kw["aggs"], AGGS, m["rows"], out["aggs"], out["agg_layout"], "search_request")
    collapse_ref.assert_same_arrays(out["collapse"], R.collapse_arrays(page, W["grp_column"], COLLAPSE, RW.SORT2, W["fields"]),
                                    "search_request")
    plain = W["ix"].search_request(*W["qs"], 11)
    assert sorted(plain) == ["count", "doc", "score", "seg"]


# ---- chains --------------------------------------------------------------------------------------------------------------
def test_chains(B):
    W = B
    check(W, "bool_tree + fscore + sort + aggs + collapse", clause="bool_tree", fscore=True, sort=RW.SORT2, aggs=AGGS,
          collapse=COLLAPSE, k=33)
    m = matched(W, "phrase", script=True)
    after = [4 if int(n) > 4 else None for n in m["matched"]]
    check(W, "phrase + script + cursor + collapse", clause="phrase", script=True, after=after, collapse=COLLAPSE, k=33)


# ---- edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 11, 257])
def test_k_edges(B, k):
    W = B
    check(W, f"bool x aggs k={k}", clause="bool", aggs=AGGS, k=k, collapse=dict(COLLAPSE, group_limit=1))


def test_a_clause_that_rejects_everything_and_queries_without_a_kind(W):
    out = check(W, "bool x fscore x aggs", clause="bool", fscore=True, aggs=AGGS, q_filter=[-1, 0, 1] * 4)
    assert int(out["got"][3][6]) == 0 and int(out["m"]["scored"][6]) == 0  # the clause stage rejects everything
    assert W["bool"][5] == ([], 0) and W["fscore"][9] is None              # queries without a kind, in the same batch
    assert int(out["got"][3][5]) == 11 and int(out["got"][3][9]) == 11


def test_two_runs_of_one_batch(B):
    W = B
    check(W, "two runs", clause="bool", fscore=True, aggs=AGGS, collapse=COLLAPSE, sort=RW.SORT2, runs=2)
    check(W, "two runs, top_hits", clause="phrase", extra=TOP_HITS, runs=2)


def test_two_batches_in_flight(W):
    import torch
    ix, qs = W["ix"], W["qs"]
    # each request alone against request_ref first: what the solo runs below give is then a checked answer
    check(W, "solo: bool x fscore x aggs", clause="bool", fscore=True, aggs=AGGS)
    check(W, "solo: bool_tree x script x sort x aggs", clause="bool_tree", script=True, sort=RW.SORT2, aggs=AGGS)
    specs = [dict(stage_args(W, "bool", True, False, "outer"), aggs=plan_of(W, AGGS, None)),
             dict(stage_args(W, "bool_tree", False, True, "outer"), aggs=plan_of(W, AGGS, None), sort=ids_of(RW.SORT2))]
    wants = []
    for kw in specs:
        with ix.prepare_request(*qs, 11, **kw) as b:
            wants.append(fetched(b, W))
    streams = [torch.cuda.Stream() for _ in specs]
    batches = [ix.prepare_request(*qs, 11, **kw) for kw in specs]
    for b, s in zip(batches, streams):
        b.set_stream(s.cuda_stream)
    for _ in range(3):
        for b in batches:
            b.run()
    for b, want in zip(batches, wants):
        got = fetched(b, W)
        assert all(x == y for x, y in zip(got, want)), "in flight"
        b.close()


def test_a_batch_keeps_its_index_state(oracle):
    """prepared before slg_index_update_deleted: the batch answers against the state it was prepared on"""
    import searchlite_amd as sa
    from tests import fscore_ref
    w = RW.build()
    w["oracle"] = oracle
    w["cands"] = fscore_ref.all_candidates(oracle, w["segs"], *w["qs"])
    ix = w["ix"] = sa.GpuIndex([copy.copy(s) for s in w["segs"]], tuning={"updatable": 1})
    try:
        w["agg_fields"] = register(w, ix)
        m = matched(w, "bool", fscore=True)
        kw = dict(stage_args(w, "bool", True, False, "outer"), aggs=plan_of(w, AGGS, None))
        with ix.prepare_request(*w["qs"], 11, **kw) as b:
            dead = np.random.default_rng(3).random(RW.SIZES[0]) < 0.4
            ix.update_deleted(0, np.packbits(dead, bitorder="little"), float(RW.SIZES[0] - int(dead.sum())))
            b.run()
            same(b.fetch()[:4], R.as_arrays(m["rows"], 11), "prepared before the update")
            assert b.matched_counts().tolist() == m["matched"].tolist()
            check_aggs(w, kw["aggs"], AGGS, m["rows"], b.aggs(), b.agg_layout(), "prepared before the update")
    finally:
        ix.close()


def test_regions_of_1_64_65_candidates_into_the_agg_walk(oracle):
    """one slice per query; regions of 1, 64 and 65 candidates that the clause stage leaves with 0, 1 and 64 survivors,
    which the aggregation walk, top_hits and collapse then read"""
    import searchlite_amd as sa
    from searchlite_amd import aggs as A
    from tests import bool_ref, fscore_ref
    from tests.util import _append_lists, random_segment
    rng = np.random.default_rng(41)
    n, vocab = 700, 20
    c64 = np.sort(rng.choice(n, 64, replace=False)).astype(np.uint32)
    rest = np.setdiff1d(np.arange(n), c64)
    lists = {"c1": c64[:1], "c64": c64, "c65": np.sort(np.append(c64, rest[0])).astype(np.uint32),
             "none": rest[1:200].astype(np.uint32), "one": np.sort(np.append(rest[200:300], c64[0])).astype(np.uint32),
             "all64": np.sort(np.concatenate([c64, rest[300:400]])).astype(np.uint32)}
    seg = _append_lists(random_segment(rng, n, vocab, 6), [(d, np.ones(len(d), np.int64)) for d in lists.values()])
    T = {name: vocab + i for i, name in enumerate(lists)}
    cases = [("c1", "none", 0), ("c1", "one", 1), ("c64", "none", 0), ("c64", "one", 1), ("c64", "all64", 64),
             ("c65", "none", 0), ("c65", "one", 1), ("c65", "all64", 64)]
    qs = RW.csr([[(T[a], 1.0 + 0.25 * i)] for i, (a, _, _) in enumerate(cases)], 1)
    cl = bool_ref.clauses_of([([(RW.MUST, [T[b]])], 0) for _, b, _ in cases], 1)
    tag = [[[RW.TAG_KEYS[int(j)] for j in rng.integers(0, 8, int(rng.integers(0, 3)))] for _ in range(n)]]
    frac = [[[float(rng.integers(-999, 999)) / 64.0] for _ in range(n)]]
    grp = [[[int(rng.integers(0, 5))] for _ in range(n)]]
    cands = fscore_ref.all_candidates(oracle, [seg], *qs)
    m = R.matched_sets(cands, [seg], len(cases), ("bool", cl))
    assert np.asarray(cands[3]).tolist() == [1, 1, 64, 64, 64, 65, 65, 65]
    assert m["clause_kept"].tolist() == [c for _, _, c in cases]
    w = dict(cols={"tag": tag, "frac": frac}, masks={}, keys_of={"tag": RW.TAG_KEYS})
    request = {"t": {"type": "terms", "field": "tag", "aggs": {"s": {"type": "stats", "field": "frac"}}}}
    with sa.GpuIndex([seg]) as ix:
        ord_of = {k_: i for i, k_ in enumerate(RW.TAG_KEYS)}
        fields = {"tag": {"id": ix.add_agg_keyword_field([[np.array([ord_of[v] for v in d], np.uint32) for d in tag[0]]], 8),
                          "keys": RW.TAG_KEYS},
                  "frac": {"id": ix.add_agg_field(frac, np.float64)}}
        gid = ix.add_agg_keyword_field([[np.array(d, np.uint32) for d in grp[0]]], 5)
        plan = A.agg_spec(dict(request, **TOP_HITS), fields)
        for k in (11, 65):
            with ix.prepare_request(*qs, k, clauses=cl, aggs=plan, collapse=dict(field=gid, group_limit=5, inner_size=2)) as b:
                assert b.info()["n_slices"] == len(cases)  # a region is a slice
                b.run()
                got = b.fetch(want_stats=True)
                page = R.as_arrays(m["rows"], k)
                same(got[:4], page, f"regions k={k}")
                assert [int(got[4][q].scored_docs) for q in range(len(cases))] == m["scored"].tolist()
                assert b.matched_counts().tolist() == m["matched"].tolist()
                want_layout, want_tables, _ = R.agg_tables(request, plan.nodes, w["cols"], {}, w["keys_of"], m["rows"])
                for g, wt in zip(b.aggs(), want_tables):
                    same_bytes(g, wt.astype(g.dtype), f"regions k={k}: tables")
                th = b.top_hits()["nodes"][0]
                for q, (total, hits) in enumerate(R.top_hits_root(m["rows"], 3, 0, [("_score", "desc")], {})):
                    nh = int(th["count"][q, 0])
                    assert [(0, int(d)) for d in th["doc"][q, 0, :nh]] == [(s, d) for s, d, _ in hits]
                want = collapse_ref.expected_arrays(*page, grp, 5, 0, 2, None, None, {})
                collapse_ref.assert_same_arrays(b.collapse_groups(), want, f"regions k={k}")


def test_sharded_runs_refuse_a_compound_batch(W):
    from searchlite_amd import _native as N, searcher
    with W["ix"].prepare_request(*W["qs"], 11, **dict(stage_args(W, "bool", True, False, "outer"), aggs=plan_of(W, AGGS, None))) as b:
        group = searcher.ShardGroup(W["ix"], 0, 1, searcher.shard_unique_id(), W["n_segs"])
        try:
            with pytest.raises(N.SlgError) as ei:
                b.run_sharded(group)
            assert ei.value.code == N.ERR_UNSUPPORTED
            with pytest.raises(N.SlgError) as ei:
                b.fetch_sharded()
            assert ei.value.code == N.ERR_UNSUPPORTED
        finally:
            group.close()


def test_sort_and_cursor_errors_behind_the_index(W):
    """a sort spec and a cursor are checked against the index, behind the NULL-index check (as in their own prepare
    calls): through the request they report the code and message the legacy entry reports"""
    from searchlite_amd import _native as N

    def error_of(prepare, **kw):
        with pytest.raises(N.SlgError) as ei:
            prepare(*W["qs"], 11, **kw)
        return ei.value.code, ei.value.msg
    bad_cursor = N.SortCursor()
    bad_cursor.has_cursor, bad_cursor.missing_mask = 1, 0xF0  # missing bits beyond the sort's parts
    cases = [dict(sort=[(0, "asc")] * 5), dict(sort=[(99, "asc")]), dict(sort=[(0, "asc")], cursors=[bad_cursor] * W["nq"]),
             dict(cursors=[((None,), 0, 0)] * W["nq"])]
    seen = set()
    for kw in cases:
        old = error_of(W["ix"].prepare, **kw)
        new = error_of(W["ix"].prepare_request, **dict(kw, **RW.clause_of(W, "bool")[1]))
        assert old == new and old[0] in (N.ERR_INVALID, N.ERR_UNSUPPORTED), (kw, old, new)
        seen.add(old[1])
    assert len(seen) >= 3  # (different faults, not one message for everything)
