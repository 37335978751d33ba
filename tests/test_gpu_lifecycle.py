"""Index updates with every kind of registered resource (searchlite_amd/csrc/slg_index.hip: update_state, copy_state,
reshape_per_segment, finish_state, slg_index_update_deleted / _add_segment / _remove_segment).

Every scenario starts from a fresh four-segment index (tuning updatable = 1) with everything of
tests/lifecycle_world.py registered: positions and a dictionary per segment, a ranked numeric column, a keyword column,
one filter from each of the four constructors, an i64 and an f64 sort field, the embedded vector store and an extra
vector field, and what was added since: a text field (one segment without text), two nested paths (two levels), a
nested keyword and a nested i64 column, a nested filter tree, a timestamp column.  The steps go to the live index and to the model together, and at each checkpoint EVERY kind of request
is checked two ways:

  (a) against lifecycle_world.expect(model, kind) with the comparison helper of the kind's own test module, at that
      module's bar: integers and f32 bit patterns exactly (plain, sorted, cursor, bool, tree, phrase, fscore, script,
      scan, aggs, collapse, rescore, expand; date_aggs, top_hits, composite page one and two, term_buckets, the compound
      request, the nested tree as bitmap / q_filter / scan filter, regex, suggest, highlight from host hits and from a
      batch), test_gpu_vector_search.check / test_gpu_hybrid.check / tests.util.check_rerank_result for the vector
      kinds.  No tolerance is introduced here;
  (b) bit for bit against a TWIN: a new GpuIndex over the model's current segment list with every resource
      registered from scratch — the header's contract ("bit-identical to a fresh slg_index_create on the updated
      descriptor").

tests/test_lifecycle_world.py shows on the CPU that no (scenario, kind) pair can pass vacuously and that each kind
would notice an unshifted resource list.

Where to find what (resource x step -> test):
  update_deleted            test_delete, test_remove_then_delete_on_the_shifted_ordinal
  remove first/middle/last  test_remove[first|middle|last], test_compaction
  add_segment               test_add (refusals one by one, then registered again), test_compaction
  batches keep their state  test_prepared_batches_keep_their_state[remove|add]
and every checkpoint of every test runs all kinds, so each resource (filters of the four constructors, sort columns,
numeric column and ranks, keyword column, positions, dictionaries, extra vector field, embedded store, d_doc_base,
deleted) has a consumer at each of them: lifecycle_world.READS.  The resources added since, and who reads them:
  text field (TextFieldHost::per_seg, d_tsegs)      highlight, highlight_batch; NO_TEXT after add: test_add; a retired
                                                    state's texts and rows: test_prepared_batches_keep_their_state
  nested paths and columns, the nested tree         nested (check_filters: its bitmap takes new tombstones with no
                                                    second registration); refusals after add: test_add
  timestamp column                                  date_aggs (with num under it and the tree filter as a source)
  suggest table (d_suggest_segs), dictionaries      suggest, regex; refused after add until set_terms: test_add
  keyword / numeric / sort columns, bitmap filter   top_hits, composite (after-key kept across an update:
                                                    test_prepared...), term_buckets (background counted at prepare:
                                                    test_prepared...[remove]), request"""
import copy

import numpy as np
import pytest

from tests import collapse_ref
from tests import lifecycle_world as W
from tests import suggest_ref
from tests import top_hits_ref
from tests.test_gpu_composite import assert_same_response as same_composite, check_raw as check_composite_raw
from tests.test_gpu_request import check_aggs as check_request_aggs
from tests.test_gpu_term_buckets import check_node as check_term_bucket_node
from tests.test_gpu_agg_date import check as check_date_tables
from tests.test_gpu_agg_values import check_value_tables
from tests.test_gpu_bool import same
from tests.test_gpu_collapse import same_rows
from tests.test_gpu_cursor import check_row
from tests.test_gpu_hybrid import check as check_hybrid
from tests.test_gpu_rescore import same as same_rescore
from tests.test_gpu_sort import check as check_sorted
from tests.test_gpu_vector_search import check as check_vector
from tests.util import assert_same_hits, check_rerank_result

pytestmark = pytest.mark.gpu
FILTERS = W.FILTER_CYCLE


@pytest.fixture(scope="module")
def sa():
    import searchlite_amd as s
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return s


# ---- a live index with everything of the model registered ------------------------------------------------------
class Live:
    def __init__(self, sa, m):
        self.sa = sa
        self.ix = sa.GpuIndex([copy.copy(s) for s in m.segs], tuning={"updatable": 1})
        self.ids = {}
        try:
            self.set_text(m, range(m.n_segs))
            self.register(m)
        except Exception:
            self.ix.close()
            raise

    def set_text(self, m, segs):
        for s in segs:
            self.ix.set_positions(s, m.segs[s].pos_offsets, m.segs[s].positions)
            self.ix.set_terms(s, m.keys[s])

    def register(self, m):
        """columns, filters, sort fields and the extra vector field, in the order that gives a fresh index
        lifecycle_world.CANON"""
        ix, ids = self.ix, self.ids
        ids["num"] = ix.add_agg_field(m.num, np.int64)
        self.n_ranks = ix.rank_agg_field(ids["num"])
        ids["kw"] = ix.add_agg_keyword_field(m.kw, len(W.KEYS))
        ids["f_mask"] = ix.add_filter(m.mask)
        ids["f_range"] = ix.add_filter_range(m.rcol, W.LO, W.HI)
        ids["f_terms"] = ix.add_filter_terms(W.term_filter_rows(m), True)
        ids["f_tree"], = ix.add_filter_trees([W.tree_program(ids)])
        ids["si"] = ix.add_sort_field(m.si, np.int64)
        ids["sf"] = ix.add_sort_field(m.sf, np.float64)
        ids["xvec"] = ix.add_vector_field(m.xvec)
        # the resources added since, behind the others: the ids above keep their values
        ids["ts"] = ix.add_agg_field(m.ts, np.int64)
        ids["numf"] = ix.add_agg_field(W.num_as_f64(m), np.float64)   # (the composite's histogram source reads f64)
        ids["text"] = ix.add_text_field(m.text)
        self.register_nested(m, ("p_c", "p_cr"), ("n_author", "n_n"))
        ids["f_nested"], = ix.add_nested_filter_trees([W.nested_program(ids)])

    def register_nested(self, m, paths, fields):
        """the nested paths (c, then c.r under it) and the nested columns, any part of them"""
        ix, ids, arrays = self.ix, self.ids, W.nested_arrays(m)
        if "p_c" in paths:
            ids["p_c"] = ix.add_nested_path(arrays["c"])
        if "p_cr" in paths:
            ids["p_cr"] = ix.add_nested_path(arrays["cr"], ids["p_c"])
        if "n_author" in fields:
            ids["n_author"] = ix.add_nested_keyword_field(ids["p_c"], arrays["author"], len(W.AUTHORS))
        if "n_n" in fields:
            ids["n_n"] = ix.add_nested_field(ids["p_cr"], arrays["n"], np.int64)

    def unregister(self):
        """(a vector field has no removal: the second registration adds a new one)"""
        self.ix.remove_filter(self.ids["f_nested"])
        for name in ("n_author", "n_n"):
            self.ix.remove_nested_field(self.ids[name])
        for name in ("p_cr", "p_c"):
            self.ix.remove_nested_path(self.ids[name])
        self.ix.remove_text_field(self.ids["text"])
        for name in ("ts", "numf"):
            self.ix.remove_agg_field(self.ids[name])
        for name in FILTERS:
            self.ix.remove_filter(self.ids[name])
        for name in ("si", "sf"):
            self.ix.remove_sort_field(self.ids[name])
        for name in ("num", "kw"):
            self.ix.remove_agg_field(self.ids[name])

    def apply(self, m, op):
        """one step on the live index and on the model together"""
        if op[0] == "delete":
            bitmap, live_docs = m.delete(op[1], op[2])
            self.ix.update_deleted(op[1], bitmap, live_docs)
        elif op[0] == "add":
            assert self.ix.add_segment(copy.copy(op[1]["segs"])) == m.add(op[1])
        else:
            self.ix.remove_segment(op[1])
            m.remove(op[1])

    def close(self):
        self.ix.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- one request per kind ----------------------------------------------------------------------------------------
def prepare(ix, kind, req):
    if kind == "scan":
        return ix.prepare_scan(req["queries"], req["k"], q_filter=req["q_filter"])
    if kind == "request":
        return ix.prepare_request(*req["q"], req["k"], **{n: v for n, v in req.items() if n not in ("q", "k")})
    return ix.prepare(*req["q"], req["k"], **{n: v for n, v in req.items() if n not in ("q", "k")})


def collect(kind, b):
    out = b.fetch()
    if kind in ("sorted", "scan"):
        out += (b.matched_counts(),)
    elif kind == "cursor":
        out += (b.matched_counts(), b.cursor_seen())
    elif kind in ("aggs", "date_aggs"):
        out += (b.matched_counts(), b.aggs(), b.agg_layout())
    elif kind == "top_hits":
        out += (b.matched_counts(), b.top_hits(), b.aggs(), b.top_hits_layout())
    elif kind == "composite":
        out += (b.matched_counts(),) + composite_pages(b)
    elif kind == "term_buckets":
        out += (b.matched_counts(), b.term_buckets(), b.term_buckets_layout())
    elif kind == "request":
        out += (b.matched_counts(), b.aggs(), b.agg_layout(), b.collapse_groups())
    elif kind == "collapse":
        out += (b.collapse_groups(),)
    elif kind == "rescore":
        out += b.rescore_details()
    return out


def shaped_pages(b):
    """(shaping reads the plan's names, keys and intervals, no id: the canonical plan serves every index)"""
    from searchlite_amd import aggs as A
    lay, page = b.composite_layout(), b.composite()
    check_composite_raw(page, lay, "composite")
    return page, [A.shape_composite(W.composite_plan(W.CANON), lay, page, q) for q in range(W.NQ)]


def set_after(b, afters):
    """page two starts behind page one's after-key; a query whose page one was its last is parked above every key"""
    from searchlite_amd import aggs as A
    lay = b.composite_layout()
    b.set_composite_after([1 << lay["key_bits"] if a is None else A.composite_lower_bound(lay, W.composite_plan(W.CANON), a)
                           for a in afters])


def composite_pages(b):
    """of a batch that has just run from the start: page one, then page two from page one's after-key (a second run);
    the batch is left as it was, at the start -> (raw pages, shaped pages)"""
    raw1, one = shaped_pages(b)
    set_after(b, [p.get("after_key") for p in one])
    b.run()
    raw2, two = shaped_pages(b)
    b.set_composite_after(None)
    return [raw1, raw2], [one, two]


def request(m, kind, ids, oracle):
    return W.cursor_request(m, oracle, ids) if kind == "cursor" else W.request(m, kind, ids)


def run(ix, kind, req):
    if kind in W.PREPARED:
        with prepare(ix, kind, req) as b:
            b.run()
            return collect(kind, b)
    if kind in ("expand", "regex"):
        return ix.expand(req["requests"])
    if kind == "suggest":
        return [suggest_ref.bits(o) for o in ix.suggest(req["requests"])]
    if kind == "highlight":
        return ix.highlight(req["hits"], req["specs"])
    if kind == "highlight_batch":
        with ix.prepare(*req["q"], req["k"]) as b:
            b.run()
            return b.fetch(), b.highlight(req["specs"])
    if kind == "nested":
        out = dict(bitmaps=ix.fetch_filter(req["filter"]))
        with prepare(ix, "bool", req["bool"]) as b:
            b.run()
            out["bool"] = b.fetch()
        with prepare(ix, "scan", req["scan"]) as b:
            b.run()
            out["scan"] = collect("scan", b)
        return out
    if kind == "vector":
        return ix.vector_search(req["clause_field"], req["qvecs"], req["alpha"], req["cand"], req["k_out"], boost=req["boost"])
    if kind == "hybrid":
        return ix.search_hybrid(*req["q"], req["k"], req["clause_field"], req["qvecs"], req["alpha"], req["cand"],
                                req["k_out"], boost=req["boost"])
    assert kind == "rerank"
    return ix.rerank_fields_batch(req["clause_field"], req["qvecs"], req["alpha"], req["cand_doc"], req["cand_seg"],
                                  req["cand_bm25"], req["cand_count"], req["k_out"], boost=req["boost"])


def check(kind, got, want, m, what):
    """(a): the kind's own comparison helper, at its own bar"""
    what = f"{what} / {kind}"
    if kind == "plain":
        assert_same_hits(got, want, 0.0, what)
        same(got, want, what)
    elif kind == "sorted":
        check_sorted(got, want, W.K, W.SORT, what)
    elif kind == "cursor":
        for q in range(W.NQ):
            check_row(got, q, want["rows"][q], want["cursors"][q], W.PAGE + 1, W.SORT, W.sort_fields(m), what=what)
    elif kind in ("bool", "tree", "phrase", "fscore", "script"):
        same(got, want, what)
    elif kind == "scan":
        same(got[:4], want["rows"], what)
        assert got[4].tolist() == want["matched"].tolist(), f"{what}: matched"
    elif kind == "aggs":
        same(got[:4], want["rows"], what)   # (the rows of an aggregation batch are those of the plain batch)
        assert got[4].tolist() == [len(d) for d in want["docs"]], f"{what}: matched"
        check_value_tables(W.agg_plan(W.CANON), W.AGGS, want["cols"], want["docs"], got[5], got[6], what, W.KEYS_OF)
    elif kind == "collapse":
        same_rows(got[:4], want["rows"], what)
        collapse_ref.assert_same_arrays(got[4], want["groups"], what)
    elif kind == "rescore":
        same_rescore(got, want, what)
    elif kind == "date_aggs":
        same(got[:4], want["rows"], what)   # (the rows of an aggregation batch are those of the plain batch)
        assert got[4].tolist() == [len(d) for d in want["docs"]], f"{what}: matched"
        check_date_tables(W.date_plan(W.CANON), got[5], got[6], want["want"], what)
    elif kind == "top_hits":
        same(got[:4], want["rows"], what)
        assert got[4].tolist() == want["matched"], f"{what}: matched"
        th, tables, lay = got[5], got[6], got[7]
        assert not th["status"].any() and [x["lists"] for x in lay] == [w_["count"].shape[1] for w_ in want["lists"]], what
        top_hits_ref.assert_same_lists(th["nodes"], want["lists"], what)
        for nd, tot in zip(W.top_hits_plan(W.CANON).top_hits_nodes, want["totals"]):
            if nd["parent"] < 0:
                assert tot[:, 0].tolist() == got[4].tolist(), f"{what}: a root's total is the matched count"
            else:
                assert np.array_equal(tot, tables[nd["parent"]][:, 0, :]), f"{what}: a child's total is the parent's count cell"
    elif kind == "composite":
        same(got[:4], want["rows"], what)
        assert got[4].tolist() == want["matched"], f"{what}: matched"
        for page in (0, 1):
            for q in range(W.NQ):
                same_composite(got[6][page][q], want["pages"][page][q], f"{what}: page {page + 1} of query {q}")
    elif kind == "term_buckets":
        same(got[:4], want["rows"], what)
        assert got[4].tolist() == want["matched"], f"{what}: matched"
        plan = W.term_buckets_plan(W.CANON)
        for nd, nlay, ngot in zip(plan.term_buckets["nodes"], got[6]["nodes"], got[5]["nodes"]):
            check_term_bucket_node(want, W.TERM_BUCKETS[nd["name"]], nd, nlay, ngot, want["nodes"][nd["name"]], f"{what}: {nd['name']}")
    elif kind == "request":
        same(got[:4], want["page"], what)
        assert got[4].tolist() == want["matched"].tolist(), f"{what}: matched"
        world = dict(cols=W.agg_columns(m), masks=m.filter_masks(), keys_of=W.KEYS_OF, nq=W.NQ)
        check_request_aggs(world, W.compound_request(m, W.CANON)["aggs"], W.REQUEST_AGGS, want["sets"], got[5], got[6], what)
        collapse_ref.assert_same_arrays(got[7], want["collapse"], what)
    elif kind == "nested":
        assert len(got["bitmaps"]) == m.n_segs
        for s in range(m.n_segs):
            assert np.array_equal(got["bitmaps"][s], want["bitmaps"][s]), f"{what}: bitmap of segment {s}"
        same(got["bool"], want["bool"], f"{what} as q_filter")
        same(got["scan"][:4], want["scan"]["rows"], f"{what} as a scan's filter")
        assert got["scan"][4].tolist() == want["scan"]["matched"].tolist(), f"{what}: matched"
    elif kind == "suggest":
        assert got == want, what                          # texts, order, doc_freq and the scores' f32 bits
    elif kind == "highlight":
        assert got == want, what                          # status and the bytes of every fragment
    elif kind == "highlight_batch":
        assert_same_hits(got[0], want["rows"], 0.0, what)
        same(got[0], want["rows"], what)
        assert got[1] == want["items"], what
    elif kind in ("expand", "regex"):
        assert len(got) == len(want)
        for r, ((ids, dist), (want_ids, want_dist)) in enumerate(zip(got, want)):
            assert ids.shape == want_ids.shape and ids.shape[1] == m.n_segs, f"{what} request {r}: {ids.shape}"
            assert ids.tolist() == want_ids.tolist() and dist.tolist() == want_dist.tolist(), f"{what} request {r}"
    elif kind == "vector":
        check_vector(got, want, W.K_OUT, what)
    elif kind == "hybrid":
        check_hybrid(got, want, W.K_OUT, 2, 0, what)
    else:
        assert kind == "rerank"
        for q, query in enumerate(want["queries"]):
            check_rerank_result(want["fields"], query, "fields", W.K_OUT, tuple(a[q] for a in got), False, f"{what} q{q}")


def checkpoint(live, m, oracle, what, kinds=W.KINDS):
    """every kind on the live index against (a) the model's expectation and (b) a twin index built from scratch"""
    got = {}
    for kind in kinds:
        got[kind] = run(live.ix, kind, request(m, kind, live.ids, oracle))
        check(kind, got[kind], W.expect(m, kind, oracle), m, what)
    with Live(live.sa, m) as twin:
        assert twin.ids == W.CANON                                 # (the ids a fresh index hands out)
        assert twin.n_ranks <= live.n_ranks                       # the live rank dictionary may be a superset
        for kind in kinds:
            fresh = run(twin.ix, kind, request(m, kind, twin.ids, oracle))
            assert W.digest(got[kind]) == W.digest(fresh), f"{what} / {kind}: differs from a fresh index over the same segments"
    return got


def check_filters(live, m, what):
    """the five registered bitmaps (the nested tree's too) against the model: alive and passing, segment by segment"""
    masks = m.filter_masks()
    for name in FILTERS + ("f_nested",):
        got = live.ix.fetch_filter(live.ids[name])
        assert len(got) == m.n_segs
        for s in range(m.n_segs):
            assert np.array_equal(got[s], masks[name][s] & ~m.dead(s)), f"{what}: filter {name} segment {s}"


def refused(sa, fn, *needles):
    with pytest.raises(sa.SlgError) as ei:
        fn()
    assert ei.value.code == -1, ei.value   # SLG_ERR_INVALID
    for needle in needles:
        assert needle in str(ei.value), ei.value


# ---- the scenarios -------------------------------------------------------------------------------------------------
def test_delete(sa, oracle):
    """update_deleted on the 65-doc segment (docs 0, 31, 32, 63 and 64, the last, among them), a larger bitmap on the
    same segment, then every doc of the 33-doc segment (live_docs 0.0): the four filters reject the new tombstones
    with no second registration, positions / dictionaries / columns / ranks / vectors are kept (their kinds pass), the
    generation rose once per call and not on any registration"""
    m, steps = W.scenario("delete")
    with Live(sa, m) as live:
        assert live.ix.generation == 0                     # no registration counts
        ids = dict(live.ids)
        before = {kind: W.expect(m, kind, oracle) for kind in W.SAME_UNDER_DELETE}
        for i, (label, op) in enumerate(steps):
            live.apply(m, op)
            assert live.ix.generation == i + 1
            got = checkpoint(live, m, oracle, label)
            check_filters(live, m, label)
            assert live.ids == ids and live.ix.rank_agg_field(ids["num"]) == live.n_ranks
            for kind in W.SAME_UNDER_DELETE:               # a dictionary and a rerank see no tombstone
                check(kind, got[kind], before[kind], m, f"{label}: unchanged by tombstones")
        assert m.segs[2].docs == 0.0 and live.ix.generation == 3
        assert live.ix.info()["n_segs"] == 4


@pytest.mark.parametrize("which", ["first", "middle", "last"])
def test_remove(sa, oracle, which):
    """remove_segment with nothing registered again: every kind answers for the three segments left (expand rows
    have three columns, vector-only search's flat doc ids follow the new d_doc_base, cardinality and percentiles are
    exact over a rank dictionary that is now a superset, and a histogram's dense id range is that of the segments
    left: the first and the last segment each hold an end of the numeric column's value range alone)"""
    m, steps = W.scenario(f"remove_{which}")
    with Live(sa, m) as live:
        ids = dict(live.ids)
        for label, op in steps:
            live.apply(m, op)
        assert live.ix.generation == 1 and live.ix.info()["n_segs"] == 3 and live.ids == ids
        got = checkpoint(live, m, oracle, f"remove {which}")
        assert all(rows.shape[1] == 3 for rows, _ in got["expand"] + got["regex"])
        check_filters(live, m, f"remove {which}")
        refused(sa, lambda: live.ix.remove_segment(3), "no such segment")


def test_remove_then_delete_on_the_shifted_ordinal(sa, oracle):
    """remove_segment(0), then update_deleted(1, ...): the segment that used to be ordinal 2.  The filters' bitmaps,
    the scan, the aggregations and vector search (every kind) see the tombstones on that segment and on no other"""
    m, steps = W.scenario("remove_then_delete")
    with Live(sa, m) as live:
        for label, op in steps:
            dead_before = [m.dead(s) for s in range(m.n_segs)]
            live.apply(m, op)
            checkpoint(live, m, oracle, label)
            check_filters(live, m, label)
        assert op[0] == "delete" and op[1] == 1 and m.n_docs()[1] == W.SIZES[2]
        for s in range(m.n_segs):   # the model's tombstones changed on ordinal 1 only (check_filters held the device to it)
            assert np.array_equal(m.dead(s), dead_before[s]) == (s != 1)
        assert live.ix.generation == 2


def test_add(sa, oracle):
    """append the fifth segment: every resource that predates it is refused or empty as the header says, one by one;
    registered again (and set_positions / set_terms for the new segment), every kind equals (a) and (b)"""
    m, steps = W.scenario("add")
    with Live(sa, m) as live:
        ix, old = live.ix, dict(live.ids)
        live.apply(m, steps[0][1])                          # (asserts the returned ordinal: 4)
        assert m.n_segs == 5 and ix.generation == 1 and ix.info()["n_segs"] == 5
        Q = W.text_queries(m)
        for name in FILTERS:                                # named filters: no bitmap for segment 4
            refused(sa, lambda: ix.search_batch(*Q, W.K, q_filter=np.full(W.NQ, old[name], np.int32)))
        refused(sa, lambda: run(ix, "bool", request(m, "bool", old, oracle)), "unknown filter id")
        refused(sa, lambda: run(ix, "tree", request(m, "tree", old, oracle)), "unknown filter id")   # as a leaf too
        for kind in ("sorted", "aggs", "collapse"):         # sort field, agg field, collapse column
            refused(sa, lambda: run(ix, kind, request(m, kind, old, oracle)), "no column for segment 4")
        refused(sa, lambda: run(ix, "expand", request(m, "expand", old, oracle)), "segment 4")
        # answers, not refusals: no positions, no vectors in the extra field
        bare = W.without_registration(m, 4)
        got = run(ix, "phrase", request(m, "phrase", old, oracle))
        check("phrase", got, W.expect(bare, "phrase", oracle), bare, "before set_positions")
        assert not any((got[1][q, :int(got[3][q])] == 4).any() for q in range(W.NQ))
        got = run(ix, "vector", request(m, "vector", old, oracle))
        check("vector", got, W.expect(bare, "vector", oracle), bare, "extra field without segment 4")
        lists = [maps for _, _, maps in W.expect(bare, "vector", oracle)]
        # (check() held `total`, the size of the union of both clauses' lists, to the reference's, whose list of the
        #  embedded store holds docs of segment 4 and whose list of the extra field holds none)
        assert any(s == 4 for mp in lists for s, _ in mp[0]) and not any(s == 4 for mp in lists for s, _ in mp[1])
        for kind in ("plain", "rescore"):                   # and what reads the segments alone is complete already
            check(kind, run(ix, kind, request(m, kind, old, oracle)), W.expect(m, kind, oracle), m, "after add_segment")
        # the resources added since, one by one, as include/searchlite_gpu.h has them
        # an aggregation field ("gives the new segment none"): the date aggregations are refused
        # (its filter source is refused "as it is in q_filter": "unknown filter id"; without it, the column shows)
        refused(sa, lambda: run(ix, "date_aggs", request(m, "date_aggs", old, oracle)), "unknown filter id")
        dates = {n: body for n, body in W.DATE_AGGS.items() if body["type"] != "filter"}
        refused(sa, lambda: ix.search_aggs(*Q, W.K, W.date_plan(old, dates)), "no column for segment 4")
        for kind in ("top_hits", "composite", "term_buckets"):   # ("a batch that names the field then fails with
            refused(sa, lambda: run(ix, kind, request(m, kind, old, oracle)))   # SLG_ERR_INVALID", whichever it names first)
        refused(sa, lambda: run(ix, "request", request(m, "request", old, oracle)))
        # a text field: "a segment added later has no text in the field (SLG_HL_NO_TEXT) until the field is registered
        # again over all segments": an answer, in both forms
        assert bare.text[4] is None and m.text[4] is not None
        for kind in ("highlight", "highlight_batch"):
            got = run(ix, kind, request(m, kind, old, oracle))
            check(kind, got, W.expect(bare, kind, oracle), bare, "the text field without segment 4")
        hits, items = W.highlight_hits(m), run(ix, "highlight", request(m, "highlight", old, oracle))
        there = [it[0] for hq, iq in zip(hits, items) for (s, _), it in zip(hq, iq) if s == 4]
        assert len(there) >= 2 * W.NQ and all(x == (W.N.HL_NO_TEXT, []) for x in there)
        # the nested tree's filter is an ordinary filter: refused as the four above
        refused(sa, lambda: ix.search_batch(*Q, W.K, q_filter=np.full(W.NQ, old["f_nested"], np.int32)), "unknown filter id")
        refused(sa, lambda: ix.prepare_scan(W.scan_queries(old)[0], W.K, q_filter=np.full(8, old["f_nested"], np.int32)),
                "unknown filter id")
        # a nested path: "a tree naming the path is then SLG_ERR_INVALID, "nested path N has no tables for segment S""
        # (the deepest scope is looked at first: the path named is c.r)
        refused(sa, lambda: ix.add_nested_filter_trees([W.nested_program(old)]), "nested path", "has no tables for segment 4")
        # ... and a nested column ("lifecycle as the paths"): under paths registered again, the old columns are refused
        live.register_nested(m, ("p_c", "p_cr"), ())
        refused(sa, lambda: ix.add_nested_filter_trees([W.nested_program(live.ids)]), "nested field", "segment 4")
        for name in ("p_cr", "p_c"):
            ix.remove_nested_path(live.ids[name])
            live.ids[name] = old[name]
        # the dictionaries: the suggester and the regex expansion are refused until set_terms
        refused(sa, lambda: run(ix, "suggest", request(m, "suggest", old, oracle)), "segment 4 has no term dictionary")
        refused(sa, lambda: run(ix, "regex", request(m, "regex", old, oracle)), "segment 4")
        assert ix.generation == 1
        # registered again
        live.unregister()
        live.set_text(m, [4])
        live.register(m)
        assert ix.generation == 1                           # registrations are no generation
        assert live.ids["xvec"] == 2 and live.ids["num"] > old["kw"] and live.ids["si"] > old["sf"]
        checkpoint(live, m, oracle, "registered again")
        check_filters(live, m, "registered again")


def test_compaction(sa, oracle):
    """add the merged segment, register again, remove the two old segments (the second at its shifted ordinal): a
    fresh index over [kept..., merged].  Removing down to one segment is allowed; the last one stays"""
    m, steps = W.scenario("compaction")
    with Live(sa, m) as live:
        ix = live.ix
        live.apply(m, steps[0][1])
        live.unregister()
        live.set_text(m, [4])
        live.register(m)
        checkpoint(live, m, oracle, "merged added, registered again")
        for label, op in steps[1:]:
            live.apply(m, op)
        assert m.n_docs() == [300, 200, 98] and ix.generation == 3
        checkpoint(live, m, oracle, "old segments removed")
        check_filters(live, m, "old segments removed")
        for _ in range(2):
            live.apply(m, ("remove", 0))
        assert m.n_docs() == [98] and ix.info()["n_segs"] == 1
        checkpoint(live, m, oracle, "one segment left")
        refused(sa, lambda: ix.remove_segment(0), "the last segment of an index cannot be removed")
        assert ix.generation == 5


@pytest.mark.parametrize("step", ["remove", "add"])
def test_prepared_batches_keep_their_state(sa, oracle, step):
    """one batch of every prepared kind, prepared before remove_segment(1) / add_segment, run and fetched after it
    and again after two further updates have retired its state: the expectation of the state it was prepared on.
    Half of the batches are closed before the index, the others after it"""
    m, _ = W.scenario("add")
    fifth = W.build()[1]
    old = m.clone()
    live = Live(sa, m)
    try:
        want = {kind: W.expect(old, kind, oracle) for kind in W.PREPARED}
        hl_specs = request(old, "highlight_batch", live.ids, oracle)["specs"]
        hl_items = W.expect(old, "highlight_batch", oracle)["items"]     # (over the rows of the `plain` batch)
        reqs = {kind: request(old, kind, live.ids, oracle) for kind in W.PREPARED}   # (kept: a batch borrows its specs)
        batches = {kind: prepare(live.ix, kind, reqs[kind]) for kind in W.PREPARED}
        ran = prepare(live.ix, "plain", reqs["plain"])
        ran.run()                                           # in flight during the update
        batches["composite"].run()                          # page one, and the after-key set: page two comes after the update
        set_after(batches["composite"], want["composite"]["afters"])
        live.apply(m, ("remove", 1) if step == "remove" else ("add", fifth))
        batches["composite"].run()
        for q, page in enumerate(shaped_pages(batches["composite"])[1]):
            same_composite(page, want["composite"]["pages"][1][q], f"the after-key set before {step}: page two of query {q}")
        batches["composite"].set_composite_after(None)
        for kind, b in batches.items():
            b.run()
            check(kind, collect(kind, b), want[kind], old, f"prepared before {step}, run after")
        check("plain", collect("plain", ran), want["plain"], old, f"run before {step}, fetched after")
        # slg_batch_highlight: "the state is the one the batch was prepared on", its texts and its rows
        assert batches["plain"].highlight(hl_specs) == hl_items and ran.highlight(hl_specs) == hl_items
        # two further updates: the state the batches hold is two generations behind the current one
        mid = m.clone()
        if step == "remove":   # (nothing was added yet: the registrations still cover every segment)
            mid_req = request(mid, "term_buckets", live.ids, oracle)
            mid_batch = prepare(live.ix, "term_buckets", mid_req)   # prepared before the tombstones below
        live.apply(m, ("delete", 0, [0, 31, 32, 63, 64]))
        if step == "remove":
            # the background tables are counted from the tombstones of the batch's state at prepare: a batch prepared
            # before update_deleted on a segment that holds foreground keys reports the old counts, a fresh one the new
            before, new = W.expect(mid, "term_buckets", oracle), W.expect(m, "term_buckets", oracle)
            bg = lambda x: [[(b["key"], b["bg_count"]) for b in r["buckets"]] for r in x["nodes"]["sig"]]
            assert bg(before) != bg(new) and any(s == 0 for h in W.TW.hits_of(W.all_hits(mid, oracle)) for s, _, _ in h)
            mid_batch.run()
            check("term_buckets", collect("term_buckets", mid_batch), before, mid, "prepared before the tombstones: the old background")
            mid_batch.close()
            check("term_buckets", run(live.ix, "term_buckets", request(m, "term_buckets", live.ids, oracle)), new, m,
                  "prepared after the tombstones: the new background")
        live.apply(m, ("remove", 0) if step == "add" else ("add", fifth))
        assert live.ix.generation == 3
        for kind, b in batches.items():
            b.run()
            check(kind, collect(kind, b), want[kind], old, f"prepared before {step}, run two updates later")
        assert batches["plain"].highlight(hl_specs) == hl_items and ran.highlight(hl_specs) == hl_items
        # and new batches see the new state (what reads the segments alone needs no second registration)
        check("plain", run(live.ix, "plain", request(m, "plain", live.ids, oracle)), W.expect(m, "plain", oracle), m,
              "the current state")
        late = [b for i, b in enumerate(batches.values()) if i % 2]
        for i, b in enumerate(batches.values()):
            if i % 2 == 0:
                b.close()
        ran.close()
    finally:
        live.close()
    for b in late:                                          # (closed with their index: closing again is harmless)
        b.close()
