"""Index updates with every kind of registered resource (searchlite_amd/csrc/slg_index.hip: update_state, copy_state,
reshape_per_segment, finish_state, slg_index_update_deleted / _add_segment / _remove_segment).

Every scenario starts from a fresh four-segment index (tuning updatable = 1) with everything of
tests/lifecycle_world.py registered: positions and a dictionary per segment, a ranked numeric column, a keyword column,
one filter from each of the four constructors, an i64 and an f64 sort field, the embedded vector store and an extra
vector field.  The steps go to the live index and to the model together, and at each checkpoint EVERY kind of request
is checked two ways:

  (a) against lifecycle_world.expect(model, kind) with the comparison helper of the kind's own test module, at that
      module's bar: integers and f32 bit patterns exactly (plain, sorted, cursor, bool, tree, phrase, fscore, script,
      scan, aggs, collapse, rescore, expand), test_gpu_vector_search.check / test_gpu_hybrid.check /
      tests.util.check_rerank_result for the vector kinds.  No tolerance is introduced here;
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
deleted) has a consumer at each of them: lifecycle_world.READS."""
import copy

import numpy as np
import pytest

from tests import collapse_ref
from tests import lifecycle_world as W
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

    def unregister(self):
        """(a vector field has no removal: the second registration adds a new one)"""
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
    return ix.prepare(*req["q"], req["k"], **{n: v for n, v in req.items() if n not in ("q", "k")})


def collect(kind, b):
    out = b.fetch()
    if kind in ("sorted", "scan"):
        out += (b.matched_counts(),)
    elif kind == "cursor":
        out += (b.matched_counts(), b.cursor_seen())
    elif kind == "aggs":
        out += (b.matched_counts(), b.aggs(), b.agg_layout())
    elif kind == "collapse":
        out += (b.collapse_groups(),)
    elif kind == "rescore":
        out += b.rescore_details()
    return out


def request(m, kind, ids, oracle):
    return W.cursor_request(m, oracle, ids) if kind == "cursor" else W.request(m, kind, ids)


def run(ix, kind, req):
    if kind in W.PREPARED:
        with prepare(ix, kind, req) as b:
            b.run()
            return collect(kind, b)
    if kind == "expand":
        return ix.expand(req["requests"])
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
    elif kind == "expand":
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
    """the four registered bitmaps against the model: alive and passing, segment by segment"""
    masks = m.filter_masks()
    for name in FILTERS:
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
        assert all(rows.shape[1] == 3 for rows, _ in got["expand"])
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
        reqs = {kind: request(old, kind, live.ids, oracle) for kind in W.PREPARED}   # (kept: a batch borrows its specs)
        batches = {kind: prepare(live.ix, kind, reqs[kind]) for kind in W.PREPARED}
        ran = prepare(live.ix, "plain", reqs["plain"])
        ran.run()                                           # in flight during the update
        live.apply(m, ("remove", 1) if step == "remove" else ("add", fifth))
        for kind, b in batches.items():
            b.run()
            check(kind, collect(kind, b), want[kind], old, f"prepared before {step}, run after")
        check("plain", collect("plain", ran), want["plain"], old, f"run before {step}, fetched after")
        # two further updates: the state the batches hold is two generations behind the current one
        live.apply(m, ("delete", 0, [0, 31, 32, 63, 64]))
        live.apply(m, ("remove", 0) if step == "add" else ("add", fifth))
        assert live.ix.generation == 3
        for kind, b in batches.items():
            b.run()
            check(kind, collect(kind, b), want[kind], old, f"prepared before {step}, run two updates later")
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
