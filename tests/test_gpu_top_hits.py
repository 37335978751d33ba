"""The top_hits aggregation on the device (slg_batch_prepare_top_hits / slg_batch_fetch_top_hits).

Expected: the oracle run with k >= the number of docs gives every matched doc with its exact score (0.0 instead under a
field sort without a `_score` part); tests/top_hits_ref.py — TopHitsCollector restated, checked against hand-derived
tables in tests/test_top_hits_ref.py — selects from them per list, the lists of a child being the parent buckets
tests/agg_date_ref.py puts a doc in.  Bar: tolerance 0 — doc, segment, score bits, counts and status all equal, zeros
past the counts; the totals (the parent's count cells, the matched counts) equal; the batch's rows, matched counts and
aggregation tables bit-identical to the same batch without the top_hits spec.  Nothing here depends on a summation
order.  The worlds and what they must provide: tests/top_hits_world.py, tests/test_top_hits_world.py.

The lists are the one-collector lists of the header (tests/top_hits_ref.one_list); how the reference's per-segment
collect and merge relates to them is tests/test_top_hits_ref.py's.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import agg_date_ref as D
from tests import top_hits_ref as T
from tests import top_hits_world as TW
from tests.util import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return sa


def open_world(gpu, w):
    from searchlite_amd import aggs as A
    w = dict(w)
    w["ix"] = ix = gpu.GpuIndex(w["segs"])
    w["sort_ids"] = {n: ix.add_sort_field(v, np.float64 if is_f else np.int64) for n, (v, is_f) in w["fields"].items()}
    fields = {n: {"sort_id": i} for n, i in w["sort_ids"].items()}
    cols = w["cols"]
    for name, keys in TW.KEYS_OF.items():
        if name in cols:
            ord_of = {k: i for i, k in enumerate(keys)}
            fields[name] = {"id": ix.add_agg_keyword_field([[np.array([ord_of[v] for v in d], np.uint32) for d in seg]
                                                            for seg in cols[name]], len(keys)), "keys": keys}
    for name, dt in (("x", np.float64), ("ts", np.int64), ("wide", np.int64)):
        if name in cols:
            fields[name] = {"id": ix.add_agg_field(cols[name], dt)}
    w["filter_ids"] = {n: ix.add_filter(m) for n, m in w["masks"].items()}
    fields[A.FILTERS] = lambda body: w["filter_ids"][body["name"]]
    w["agg_fields"] = fields
    w["expected"] = {}
    return w


@pytest.fixture(scope="module")
def W(gpu, oracle):
    w = open_world(gpu, TW.build(oracle))
    yield w
    w["ix"].close()


def ids_of(sort, ids):
    return None if sort is None else [(p if p == "_score" else ids[p], o) for p, o in sort]


def expected(W, request, plan, hits, sort, key):
    """-> (the lists per node, the totals per node, the reference layout of the aggregation nodes), once per key"""
    if key is not None and key in W["expected"]:
        return W["expected"][key]
    layout = D.ref_layout(plan.nodes, W["cols"], TW.KEYS_OF)
    match_only = sort is not None and not any(p == "_score" for p, _ in sort)
    want, totals = T.expected(TW.ref_nodes(request, plan, layout), layout, hits, W["cols"], W["masks"], TW.KEYS_OF,
                              W["fields"], match_only=match_only)
    if key is not None:
        W["expected"][key] = (want, totals, layout)
    return want, totals, layout


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def run_case(W, request, sort=None, k=11, q_filter=None, hits=None, max_entries=0, twice=False, fail=(), key=None,
             what="", permute=None):
    """one top_hits batch against the reference and against the same batch without the spec.  sort: the batch's own
    sort by field names; hits: the matched docs per query when they are not the world's; fail: the queries whose runs
    do not fit max_entries (status 1, zero lists) -> the batch's top_hits arrays"""
    from searchlite_amd import aggs as A
    what = f"{what} sort={sort} k={k} max_entries={max_entries}"
    ix = W["ix"]
    plan = A.agg_spec(request, W["agg_fields"])
    if permute is not None:  # (agg_spec emits the nodes of one parent side by side: the C ABI takes any order)
        from searchlite_amd import _native as N
        moved = N.TopHitsSpec()
        moved.n_nodes = plan.top_hits.n_nodes
        for dst, src in enumerate(permute):
            C.memmove(C.addressof(moved.nodes[dst]), C.addressof(plan.top_hits.nodes[src]), C.sizeof(N.TopHitsNode))
        plan.top_hits, plan.top_hits_nodes = moved, [plan.top_hits_nodes[src] for src in permute]
    plan.top_hits.max_entries = max_entries
    hits = W["hits"] if hits is None else hits
    want, totals, _ = expected(W, request, plan, hits, sort, key)
    q = (W["offs"], W["terms"], W["w"])
    kw = dict(sort=ids_of(sort, W["sort_ids"]), q_filter=q_filter)
    has_aggs = plan.spec.n_nodes > 0
    with ix.prepare(*q, k, aggs=plan, **kw) as b:
        b.run()
        rows, matched, got = b.fetch(), b.matched_counts(), b.top_hits()
        tables = b.aggs() if has_aggs else []
        lay = b.top_hits_layout()
        if twice:
            b.run()
            again = b.top_hits()
            same(again["status"], got["status"], what + " second run: status")
            T.assert_same_lists(again["nodes"], got["nodes"], what + " second run")
            for a, b_ in zip(b.fetch(), rows):
                same(a, b_, what + " second run: rows")
    # the invariant: rows, matched counts and every table as without the spec
    if has_aggs:
        *base, base_matched, base_tables, _ = ix.search_aggs(*q, k, plan.spec, **kw)
        same(matched, base_matched, what + ": matched vs the aggregation batch")
        assert len(tables) == len(base_tables)
        for i, (a, b_) in enumerate(zip(tables, base_tables)):
            same(a, b_, f"{what}: table {i} vs the aggregation batch")
    elif sort is not None:
        *base, base_matched = ix.search_sorted(*q, k, kw["sort"], q_filter=q_filter)
        same(matched, base_matched, what + ": matched vs the sorted batch")
    else:
        with ix.prepare(*q, k, q_filter=q_filter) as plain:
            plain.run()
            base = plain.fetch()
    for a, b_, name in zip(rows, base, ("doc", "seg", "score", "count")):
        same(a, b_, f"{what}: rows differ in {name} from the batch without top_hits")
    assert matched.tolist() == [len(h) for h in hits], what + ": matched"
    # the layout, the status, the lists, the totals
    at_list = at_hit = 0
    for th, x in zip(plan.top_hits_nodes, lay):
        lists = 1 if th["parent"] < 0 else tables[th["parent"]].shape[2]
        assert x == dict(lists=lists, size=th["size"], list_offset=at_list, hit_offset=at_hit), what + ": layout"
        at_list, at_hit = at_list + lists, at_hit + lists * th["size"]
    assert got["status"].tolist() == [1 if i in fail else 0 for i in range(len(hits))], what + ": status"
    if fail:  # (a copy: the expected arrays are shared between the cases of a key)
        want = [{n: a.copy() for n, a in w_.items()} for w_ in want]
        for i in fail:
            for w_ in want:
                for a in w_.values():
                    a[i] = 0
    T.assert_same_lists(got["nodes"], want, what)
    for th, tot in zip(plan.top_hits_nodes, totals):
        if th["parent"] < 0:
            assert tot[:, 0].tolist() == matched.tolist(), what + ": a root's total is the matched count"
        else:
            assert np.array_equal(tot, tables[th["parent"]][:, 0, :]), what + ": a child's total is the parent's count cell"
    return got


def hits_node(size, frm=0, sort=()):
    return {"type": "top_hits", "size": size, "from": frm, "sort": [{"field": f, "order": o} for f, o in sort]}


def terms_len(*nodes):
    return {"by_len": {"type": "terms", "field": "len", "aggs": {f"h{i}": nd for i, nd in enumerate(nodes)}}}


# L in {1, 2, 63, 64} x from in {0, 1, L - 1, >= length} over lists of 0, 1, 63, 64, 65, 128 and 129 entries
SLICES = {"L1_L2": ((0, 1), (0, 2), (1, 1)), "L63": ((0, 63), (1, 62), (62, 1)), "L64": ((0, 64), (1, 63), (63, 1))}


@pytest.mark.parametrize("name", sorted(SLICES))
def test_list_lengths_and_slices(W, name):
    """three nodes under one parent share its runs; the sorts differ, so only the select is repeated"""
    sorts = ((), (("low", "asc"),), (("n", "desc"), ("_score", "desc")))
    nodes = [hits_node(size, frm, sorts[i]) for i, (frm, size) in enumerate(SLICES[name])]
    got = run_case(W, terms_len(*nodes), key=name, what=name)
    for (frm, size), arr in zip(SLICES[name], got["nodes"]):
        assert arr["count"][0].tolist() == [min(size, max(0, n - frm)) for n in TW.LENGTHS]
    if name == "L64":
        run_case(W, terms_len(*nodes), sort=[("low", "desc"), ("_score", "desc")], key=name + " sorted", what=name)


def test_ties_fall_to_segment_then_doc(W):
    request = {"by_tag": {"type": "terms", "field": "tag", "aggs": {"a": hits_node(64, 0, (("tie", "asc"),)),
                                                                    "d": hits_node(4, 60, (("tie", "desc"),))}},
               "root": hits_node(64, 0, (("tie", "desc"),))}
    got = run_case(W, request, key="ties", what="ties")
    root = got["nodes"][2]
    pairs = list(zip(root["seg"][0, 0].tolist(), root["doc"][0, 0].tolist()))
    assert pairs == sorted((s, d) for s, d, _ in W["hits"][0])[:64]


PARENTS = {
    "terms": {"type": "terms", "field": "tag", "missing": "none"},
    "histogram": {"type": "histogram", "field": "x", "interval": 1.5, "missing": 100.0},
    "range": {"type": "range", "field": "x", "ranges": [{"to": 1.0}, {"from": -1.0}, {"from": 50.0}]},
    "date_histogram": {"type": "date_histogram", "field": "ts", "calendar_interval": "week"},
    "filter": {"type": "filter", "filter": {"name": "half"}},
}


@pytest.mark.parametrize("kind", sorted(PARENTS))
def test_parent_kinds(W, kind):
    """terms with docs holding two ordinals, a repeated ordinal and the missing row; a histogram with several values
    per doc; two overlapping ranges and an empty one; date_histogram; filter (the one-list path)"""
    body = dict(PARENTS[kind], aggs={"best": hits_node(3, 0, (("n", "asc"),)), "next": hits_node(2, 1)})
    got = run_case(W, {"p": body}, key="parent " + kind, what=kind, twice=(kind == "terms"))
    assert got["nodes"][0]["count"][0].max() == 3
    if kind == "range":
        assert got["nodes"][0]["count"][0, 2] == 0  # the empty range
        # one doc as a hit of both overlapping ranges: the smallest `n` among the docs with a value in [-1, 1]
        both = {"type": "range", "field": "x", "ranges": [{"from": -1.0, "to": 1.0}, {"from": -1.0, "to": 1.0},
                                                         {"to": 1.0}, {"from": -1.0}],
                "aggs": {"best": hits_node(1, 0, (("n", "asc"), ("_score", "desc")))}}
        arr = run_case(W, {"p": both}, key="parent range twice", what="range twice")["nodes"][0]
        hit = lambda r: (int(arr["seg"][0, r, 0]), int(arr["doc"][0, r, 0]))
        assert arr["count"][0].tolist() == [1, 1, 1, 1] and hit(0) == hit(1)
    run_case(W, {"p": body}, sort=[("low", "asc")], key="parent sorted " + kind, what=kind + " sorted")


@pytest.mark.parametrize("interval,rows", [(1, 9000), (2, 4500), (100, 90)])
def test_parent_homes_and_cursor_homes(W, interval, rows):
    """9000 rows: the parent's counts in device memory, the cursors in the scratch slice; 4500: counts in LDS, cursors
    in scratch; 90: both in LDS"""
    body = {"type": "histogram", "field": "wide", "interval": interval,
            "aggs": {"best": hits_node(2, 0, (("low", "asc"), ("_score", "desc")))}}
    got = run_case(W, {"p": body}, key=f"wide {interval}", what=f"wide {interval}", twice=(interval == 1))
    assert got["nodes"][0]["count"].shape == (12, rows)


def test_root_nodes_from_one_doc_to_every_doc(W):
    """queries of 0, 1, 40 (< a wave), ~150 (< four waves' worth) and > 2000 matched docs"""
    request = {"a": hits_node(10), "b": hits_node(1, 63, (("low", "asc"),)), "c": hits_node(64, 0, (("f64", "desc"),)),
               "d": hits_node(2, 1, (("n", "asc"),))}
    got = run_case(W, request, key="roots", what="roots", twice=True)
    n = [len(h) for h in W["hits"]]
    assert got["nodes"][0]["count"][:, 0].tolist() == [min(10, x) for x in n]
    assert got["nodes"][1]["count"][:, 0].tolist() == [1 if x > 63 else 0 for x in n]
    run_case(W, request, sort=[("n", "desc")], key="roots sorted", what="roots sorted")


def test_more_slices_than_waves(gpu, oracle):
    w = open_world(gpu, TW.build_many(oracle))
    try:
        request = {"a": hits_node(64), "b": hits_node(7, 2, (("low", "desc"),))}
        run_case(w, request, what="six segments")
        run_case(w, request, sort=[("low", "asc")], what="six segments sorted")
    finally:
        w["ix"].close()


def test_a_root_and_a_child_in_one_spec(W):
    request = {"by_tag": {"type": "terms", "field": "tag", "aggs": {"best": hits_node(3, 0, (("low", "asc"),)),
                                                                    "s": {"type": "stats", "field": "x"}}},
               "newest": hits_node(5, 0, (("n", "desc"),)),
               "wide": {"type": "histogram", "field": "wide", "interval": 1000, "aggs": {"best": hits_node(2)}}}
    run_case(W, request, key="root and child", what="root and child")


@pytest.mark.parametrize("interval", [1, 100])
def test_nodes_of_one_parent_apart_in_the_spec(W, interval):
    """parents [p0, p1, p0] and [p0, root, p0]: a query holds the runs of one parent at a time, so the third node must
    not select from what the second left (p1's cursors in the scratch slice at interval 1, in LDS over p0's at 100)"""
    p0 = {"type": "terms", "field": "tag", "missing": "none",
          "aggs": {"a": hits_node(3, 0, (("low", "asc"),)), "b": hits_node(4, 1, (("n", "desc"),))}}
    p1 = {"type": "histogram", "field": "wide", "interval": interval, "aggs": {"c": hits_node(2, 0, (("n", "asc"),))}}
    side = run_case(W, {"p0": p0, "p1": p1}, key=f"apart {interval} side by side", what="[p0, p0, p1]")
    got = run_case(W, {"p0": p0, "p1": p1}, permute=(0, 2, 1), key=f"apart {interval}", what="[p0, p1, p0]", twice=True)
    T.assert_same_lists([got["nodes"][i] for i in (0, 2, 1)], side["nodes"], "the order of the nodes changes no list")
    assert got["nodes"][2]["count"][0].min() == 4  # the third node's lists are full ones
    if interval == 1:
        run_case(W, {"p0": p0, "r": hits_node(5)}, permute=(0, 2, 1), key="apart root", what="[p0, root, p0]")
        run_case(W, {"p0": p0, "p1": p1}, permute=(2, 0, 1), sort=[("low", "asc")], key="apart sorted", what="[p1, p0, p0]")


SORTS = [(), (("f64", "asc"),), (("f64", "desc"),), (("low", "asc"), ("_score", "desc")),
         (("f64", "desc"), ("low", "asc"), ("_score", "asc"), ("n", "desc"))]


@pytest.mark.parametrize("sort", SORTS, ids=repr)
def test_node_sorts(W, sort):
    """in a score-ordered batch, in a field-sorted batch without `_score` (every hit's score is 0.0, a `_score` part
    ties everywhere) and in a field-sorted batch with a `_score` part"""
    request = {"by_tag": {"type": "terms", "field": "tag", "aggs": {"best": hits_node(5, 1, sort)}},
               "root": hits_node(5, 1, sort)}
    got = run_case(W, request, key=f"sorts {sort}", what="score order")
    assert got["nodes"][0]["score"][0].any()
    got = run_case(W, request, sort=[("low", "asc")], key=f"sorts {sort} match only", what="match only")
    assert not got["nodes"][0]["score"].any() and not got["nodes"][1]["score"].any()
    run_case(W, request, sort=[("low", "asc"), ("_score", "desc")], key=f"sorts {sort} scored", what="field sort with _score")


def test_doc_filter_and_tombstones(W, oracle):
    qf = np.full(12, -1, np.int32)
    qf[0] = qf[3] = qf[8] = W["filter_ids"]["third"]
    want = oracle.search_batch_filtered(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], qf,
                                        {W["filter_ids"]["third"]: W["masks"]["third"]}, strategy=oracle.BM25)
    hits = TW.hits_of(want)
    assert 0 < len(hits[0]) < len(W["hits"][0]) and len(hits[1]) == len(W["hits"][1])
    dead = W["segs"][1].deleted
    assert dead is not None and not any((dead[d >> 3] >> (d & 7)) & 1 for s, d, _ in hits[0] if s == 1)
    request = {"by_tag": {"type": "terms", "field": "tag", "aggs": {"best": hits_node(4, 0, (("n", "asc"),))}},
               "root": hits_node(6)}
    run_case(W, request, q_filter=qf, hits=hits, what="filtered")
    run_case(W, request, sort=[("n", "asc")], q_filter=qf, hits=hits, what="filtered sorted")


def test_k_zero(W):
    request = {"by_tag": {"type": "terms", "field": "tag", "aggs": {"best": hits_node(3)}}, "root": hits_node(3)}
    run_case(W, request, k=0, key="k0", what="k = 0")
    run_case(W, {"root": hits_node(3)}, k=0, key="k0 root", what="k = 0, roots alone")


def test_overflow_fails_one_query_alone(W):
    """max_entries just below and exactly at what query 0 needs, in a batch whose other queries fit"""
    request = {"by_tag": {"type": "terms", "field": "tag", "missing": "none",
                          "aggs": {"best": hits_node(3, 0, (("low", "asc"),))}}, "root": hits_node(2)}
    got = run_case(W, request, key="overflow", what="default capacity")
    _, totals, _ = W["expected"]["overflow"]
    need = totals[0].sum(axis=1)
    assert int(need[0]) == int(need.max()) and int(np.sort(need)[-2]) < int(need[0]) - 1
    run_case(W, request, max_entries=int(need[0]), key="overflow", what="exactly enough")
    got = run_case(W, request, max_entries=int(need[0]) - 1, fail=(0,), key="overflow", what="one entry short")
    assert not any(a[0].any() for nd in got["nodes"] for a in nd.values())  # the root's list of that query too
    assert got["nodes"][1]["count"][1:].any()


def test_rerun_and_a_smaller_batch_through_the_same_buffers(W):
    """the same batch twice (run_case: twice), then four of its queries alone: the pool hands the freed buffers to the
    smaller batch, and nothing of the larger one shows behind its counts"""
    from searchlite_amd import aggs as A
    request = {"by_len": {"type": "terms", "field": "len", "aggs": {"best": hits_node(64, 0, (("low", "asc"),))}},
               "root": hits_node(64)}
    run_case(W, request, key="rerun", what="all twelve", twice=True)
    want, _, _ = W["expected"]["rerun"]
    pick = [8, 9, 10, 11]
    offs = np.arange(5, dtype=np.uint32) * 3
    terms = np.concatenate([W["terms"][3 * q:3 * q + 3] for q in pick])
    w = np.concatenate([W["w"][3 * q:3 * q + 3] for q in pick])
    plan = A.agg_spec(request, W["agg_fields"])
    *_, hits = W["ix"].search_top_hits(offs, terms, w, 11, plan)
    assert not hits["status"].any()
    T.assert_same_lists(hits["nodes"], [{n: a[pick] for n, a in nd.items()} for nd in want], "four queries")
    assert hits["nodes"][1]["count"][:, 0].tolist() == [64, 40, 0, 1]
    assert not hits["nodes"][1]["doc"][2:, 0, 1:].any() and not hits["nodes"][0]["count"][2].any()


def test_one_shot_form_lifecycle_and_refusals(W):
    from searchlite_amd import _native as N
    from searchlite_amd import aggs as A
    ix, lib = W["ix"], W["ix"]._lib
    request = {"by_tag": {"type": "terms", "field": "tag", "aggs": {"best": hits_node(3, 0, (("low", "asc"),))}},
               "root": hits_node(4)}
    plan = A.agg_spec(request, W["agg_fields"])
    want, _, _ = expected(W, request, plan, W["hits"], None, "one shot")
    # prepare, fetch before the run, run, fetch, destroy
    with ix.prepare(W["offs"], W["terms"], W["w"], 11, aggs=plan) as b:
        assert lib.slg_batch_fetch_top_hits(b._h, None, None, None, None, None) == N.ERR_INVALID
        assert b"has not run" in lib.slg_last_error()
        b.run()
        assert lib.slg_batch_fetch_top_hits(b._h, None, None, None, None, None) == N.OK  # every array may be NULL
        T.assert_same_lists(b.top_hits()["nodes"], want, "prepared")
    # the one-shot form
    nq, n_segs = 12, 2
    keep = [(np.ascontiguousarray(W["terms"][3 * q:3 * q + 3].reshape(-1)), np.ascontiguousarray(W["w"][3 * q:3 * q + 3]))
            for q in range(nq)]
    queries = (N.Query * nq)()
    for q, (t, w_) in enumerate(keep):
        queries[q].term_ids, queries[q].weights, queries[q].n_terms = t.ctypes.data, w_.ctypes.data, 3
    rows = len(TW.KEYS)  # (no `missing`: a row per key)
    hc, lc, k = rows * 3 + 4, rows + 1, 11
    u = lambda *s: np.zeros(s, np.uint32)
    doc, seg, score, count = u(nq, k), u(nq, k), np.zeros((nq, k), np.float32), u(nq)
    matched, counts = np.zeros(nq, np.uint64), np.zeros((nq, rows), np.uint64)
    th_doc, th_seg, th_score, th_count, th_status = u(nq, hc), u(nq, hc), np.zeros((nq, hc), np.float32), u(nq, lc), u(nq)
    p = lambda a: a.ctypes.data
    rc = lib.slg_search_batch_top_hits(ix._h, C.addressof(queries), nq, None, None, None, C.addressof(plan.spec),
                                       C.addressof(plan.top_hits), k, 1, p(doc), p(seg), p(score), p(count), p(matched),
                                       p(counts), None, None, p(th_doc), p(th_seg), p(th_score), p(th_count), p(th_status))
    assert rc == N.OK, lib.slg_last_error()
    assert not th_status.any() and matched.tolist() == [len(h) for h in W["hits"]]
    cut = rows * 3
    assert np.array_equal(th_doc[:, :cut].reshape(nq, rows, 3), want[0]["doc"]) and np.array_equal(th_doc[:, cut:], want[1]["doc"][:, 0])
    assert np.array_equal(th_seg[:, :cut].reshape(nq, rows, 3), want[0]["seg"])
    assert np.array_equal(th_score[:, cut:].view(np.uint32), want[1]["score"][:, 0].view(np.uint32))
    assert np.array_equal(th_count[:, :rows], want[0]["count"]) and np.array_equal(th_count[:, rows], want[1]["count"][:, 0])
    assert np.array_equal(counts, W["expected"]["one shot"][1][0])  # the parent's count cells are the children's totals
    # a batch of another kind
    with ix.prepare(W["offs"], W["terms"], W["w"], 11, aggs=plan.spec) as b:
        b.run()
        assert lib.slg_batch_fetch_top_hits(b._h, None, None, None, None, None) == N.ERR_INVALID
        assert b"not a top_hits batch" in lib.slg_last_error()
        assert lib.slg_batch_top_hits_layout(b._h, (N.TopHitsLayout * 1)()) == N.ERR_INVALID
    # against the index: an unknown sort field, and more hit cells than a query may have
    bad = A.agg_spec({"root": hits_node(3, 0, (("low", "asc"),))}, W["agg_fields"])
    bad.top_hits.nodes[0].sort.field[0] = 12345
    with pytest.raises(N.SlgError) as ei:
        ix.prepare(W["offs"], W["terms"], W["w"], 11, aggs=bad)
    assert ei.value.code == N.ERR_INVALID and "sort field" in ei.value.msg
    big = A.agg_spec({"p": {"type": "histogram", "field": "wide", "interval": 1, "aggs": {"best": hits_node(8)}}},
                     W["agg_fields"])  # 9000 x 8 cells
    with pytest.raises(N.SlgError) as ei:
        ix.prepare(W["offs"], W["terms"], W["w"], 11, aggs=big)
    assert ei.value.code == N.ERR_UNSUPPORTED and "SLG_MAX_TOP_HITS_CELLS" in ei.value.msg


def test_recipes_quickest_per_diet(gpu, oracle):
    """the recipes corpus with the committed columns: terms on dietary_tags with the three quickest recipes of every
    tag (top_hits size 3 sorted by total_time_minutes), through search_top_hits and aggs.shape"""
    from searchlite_amd import aggs as A
    segs, z = load_golden("recipes.npz")
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    ag, so = np.load(os.path.join(gold, "recipes_aggs.npz")), np.load(os.path.join(gold, "recipes_sort.npz"))
    keys = [str(k) for k in ag["diet_keys"]]
    n = segs[0].n_docs
    csr = lambda o, v, f: [[f(x) for x in v[o[d]:o[d + 1]]] for d in range(n)]
    cols = {"dietary_tags": [csr(ag["diet_offsets"], ag["diet_ords"], lambda x: keys[int(x)])]}
    fields = {"total_time_minutes": ([csr(so["total_time_minutes_offsets"], so["total_time_minutes"], int)], False)}
    request = {"by_diet": {"type": "terms", "field": "dietary_tags",
                           "aggs": {"quickest": hits_node(3, 0, (("total_time_minutes", "asc"),))}}}
    qo, qt, qw = z["q_offsets"], z["q_terms"], z["q_weights"]
    hits = TW.hits_of(oracle.search_batch(segs, qo, qt, qw, n, strategy=oracle.BM25))
    with gpu.GpuIndex(segs) as ix:
        reg = {"dietary_tags": {"id": ix.add_agg_keyword_field([(ag["diet_offsets"], ag["diet_ords"])], len(keys)),
                                "keys": keys},
               "total_time_minutes": {"sort_id": ix.add_sort_field([(so["total_time_minutes_offsets"],
                                                                     so["total_time_minutes"])], np.int64)}}
        plan = A.agg_spec(request, reg)
        *_, matched, tables, layout, got = ix.search_top_hits(qo, qt, qw, 2, plan)
    keys_of = {"dietary_tags": keys}
    ref_layout = D.ref_layout(plan.nodes, cols, keys_of)
    want, totals = T.expected(TW.ref_nodes(request, plan, ref_layout), ref_layout, hits, cols, {}, keys_of, fields)
    assert not got["status"].any() and any(len(h) > 3 for h in hits)
    T.assert_same_lists(got["nodes"], want, "recipes")
    assert np.array_equal(totals[0], tables[0][:, 0, :])
    for q in range(len(hits)):
        resp = A.shape(plan, layout, tables, q, got, matched)
        for bucket in resp["by_diet"]["buckets"]:
            row = keys.index(bucket["key"])
            th = bucket["aggregations"]["quickest"]
            assert th["total"] == bucket["doc_count"] == int(totals[0][q, row])
            assert [(h["segment"], h["doc"]) for h in th["hits"]] == \
                [(int(s), int(d)) for s, d in zip(want[0]["seg"][q, row], want[0]["doc"][q, row])][:int(want[0]["count"][q, row])]
