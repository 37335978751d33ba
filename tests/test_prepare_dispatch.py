"""PreparedBatch.__init__ against a stub index: which slg_batch_prepare* entry each kind of batch calls, with which
arguments at which position, and the combinations the mirror refuses itself with the library's code.  No GPU and
no library: the stub records the call and hands back a handle."""
import ctypes as C

import numpy as np
import pytest

from searchlite_amd import _native as N
from searchlite_amd import searcher

NQ, K, STRATEGY, HANDLE = 3, 7, N.STRATEGY_BMW, 0x51A7


class _Lib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0xBA7C4 if name.startswith("slg_batch_prepare") else 0
        return entry


class _Index:
    def __init__(self):
        self._lib = _Lib()
        self._h = HANDLE
        self._batches = set()


OFFS = np.array([0, 1, 2, 3], dtype=np.uint32)
TERMS = np.array([4, 5, 6], dtype=np.uint32)
WEIGHTS = np.array([1.0, 2.0, 3.0], dtype=np.float32)
QF = np.array([-1, 0, -1], dtype=np.int32)
SORT = [("_score", "desc"), (2, "asc")]
CURSORS = [None, None, None]


def _agg_spec(n_nodes=1):
    s = N.AggSpec()
    s.n_nodes = n_nodes
    return s


def _offsets():
    return np.zeros(NQ + 1, dtype=np.uint32)


# one value of every argument that names a kind (the spec forms that need no further input)
GIVEN = {
    "sort": lambda: SORT,
    "cursors": lambda: CURSORS,
    "hybrid": lambda: True,
    "aggs": _agg_spec,
    "rescore": lambda: {"q_offsets": _offsets(), "window": 4},
    "clauses": lambda: {"c_offsets": _offsets(), "g_offsets": _offsets()},
    "phrases": lambda: {"p_offsets": _offsets()},
    "fscore": lambda: (N.FscoreSpec(), None),
    "collapse": lambda: (N.CollapseSpec(1, 2, 0, 3, None), None),
    "clause_tree": lambda: {"c_offsets": _offsets(), "g_offsets": _offsets(), "f_offsets": _offsets(),
                            "n_offsets": _offsets()},
    "script": lambda: (N.ScriptSpec(), None),
    "top_hits": N.TopHitsSpec,
    "composite": N.CompositeSpec,
    "term_buckets": N.TermBucketSpec,
}


def _prepare(**kinds):
    ix = _Index()
    kw = {name: GIVEN[name]() if v is True else v for name, v in kinds.items()}
    b = searcher.PreparedBatch(ix, OFFS, TERMS, WEIGHTS, K, STRATEGY, q_filter=QF, **kw)
    calls = [c for c in ix._lib.calls if c[0].startswith("slg_batch_prepare")]
    assert len(calls) == 1
    assert b in ix._batches and b._h == 0xBA7C4
    return b, calls[0][0], calls[0][1], kw


def _lead_ok(args):
    """the seven leading arguments and the two trailing ones of every prepare call"""
    assert args[0] == HANDLE and args[1] == NQ
    assert all(isinstance(a, int) and a != 0 for a in args[2:7])  # offsets, terms, weights, plans, q_filter
    assert args[-2] == K and args[-1] == STRATEGY


S, P = "set", "null"  # a pointer argument that is given / NULL

# kind -> (arguments, entry point, the pointers between q_filter and k: name and nullness)
KINDS = {
    "plain": ({}, "slg_batch_prepare_plans", []),
    "sorted": ({"sort": True}, "slg_batch_prepare_sorted", [("sort", S)]),
    "after_score": ({"cursors": True}, "slg_batch_prepare_after", [("sort", P), ("cursor", S)]),
    "after_sorted": ({"cursors": True, "sort": True}, "slg_batch_prepare_after", [("sort", S), ("cursor", S)]),
    "hybrid": ({"hybrid": True}, "slg_batch_prepare_hybrid", []),
    "aggs": ({"aggs": True}, "slg_batch_prepare_aggs", [("sort", P), ("aggs", S)]),
    "aggs_sorted": ({"aggs": True, "sort": True}, "slg_batch_prepare_aggs", [("sort", S), ("aggs", S)]),
    "rescore": ({"rescore": True}, "slg_batch_prepare_rescore", [("rescore", S)]),
    "bool": ({"clauses": True}, "slg_batch_prepare_bool", [("sort", P), ("bool", S)]),
    "bool_sorted": ({"clauses": True, "sort": True}, "slg_batch_prepare_bool", [("sort", S), ("bool", S)]),
    "phrase": ({"phrases": True}, "slg_batch_prepare_phrase", [("sort", P), ("bool", P), ("phrase", S)]),
    "phrase_bool": ({"phrases": True, "clauses": True, "sort": True}, "slg_batch_prepare_phrase",
                    [("sort", S), ("bool", S), ("phrase", S)]),
    "fscore": ({"fscore": True}, "slg_batch_prepare_fscore", [("sort", P), ("fscore", S)]),
    "fscore_sorted": ({"fscore": True, "sort": True}, "slg_batch_prepare_fscore", [("sort", S), ("fscore", S)]),
    "collapse": ({"collapse": True}, "slg_batch_prepare_collapse", [("sort", P), ("cursor", P), ("collapse", S)]),
    "collapse_after": ({"collapse": True, "cursors": True, "sort": True}, "slg_batch_prepare_collapse",
                       [("sort", S), ("cursor", S), ("collapse", S)]),
    "tree": ({"clause_tree": True}, "slg_batch_prepare_bool_tree", [("sort", P), ("tree", S)]),
    "tree_sorted": ({"clause_tree": True, "sort": True}, "slg_batch_prepare_bool_tree", [("sort", S), ("tree", S)]),
    "script": ({"script": True}, "slg_batch_prepare_script", [("sort", P), ("script", S), ("fscore", P), ("order", 0)]),
    "script_fscore": ({"script": True, "fscore": True, "sort": True, "script_order": "inner"},
                      "slg_batch_prepare_script", [("sort", S), ("script", S), ("fscore", S), ("order", 1)]),
    "top_hits": ({"top_hits": True}, "slg_batch_prepare_top_hits", [("sort", P), ("aggs", P), ("top_hits", S)]),
    "top_hits_aggs": ({"top_hits": True, "aggs": True, "sort": True}, "slg_batch_prepare_top_hits",
                      [("sort", S), ("aggs", S), ("top_hits", S)]),
    "composite": ({"composite": True}, "slg_batch_prepare_composite", [("sort", P), ("aggs", P), ("composite", S)]),
    "composite_aggs": ({"composite": True, "aggs": True, "sort": True}, "slg_batch_prepare_composite",
                       [("sort", S), ("aggs", S), ("composite", S)]),
    "term_buckets": ({"term_buckets": True}, "slg_batch_prepare_term_buckets",
                     [("sort", P), ("aggs", P), ("term_buckets", S)]),
    "term_buckets_aggs": ({"term_buckets": True, "aggs": True, "sort": True}, "slg_batch_prepare_term_buckets",
                          [("sort", S), ("aggs", S), ("term_buckets", S)]),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_every_kind_calls_its_entry_point(kind):
    kinds, entry, middle = KINDS[kind]
    b, name, args, kw = _prepare(**kinds)
    assert name == entry
    _lead_ok(args)
    assert len(args) == 7 + len(middle) + 2
    for (what, state), a in zip(middle, args[7:-2]):
        if what == "order":
            assert a == state
        elif state == P:
            assert a is None, what
        else:
            assert isinstance(a, int) and a != 0, what
    # the specs the caller handed over are the ones the library is pointed at
    at = dict(zip([w for w, _ in middle], args[7:-2]))
    for arg, what in (("aggs", "aggs"), ("top_hits", "top_hits"), ("composite", "composite"),
                      ("term_buckets", "term_buckets")):
        if arg in kw:
            assert at[what] == C.addressof(kw[arg])
    for arg, what in (("fscore", "fscore"), ("collapse", "collapse"), ("script", "script")):
        if arg in kw:
            assert at[what] == C.addressof(kw[arg][0])
    # the public attributes
    assert b.sorted == ("sort" in kinds) and b.after == ("cursors" in kinds) and b.is_hybrid == ("hybrid" in kinds)
    assert b.is_rescore == ("rescore" in kinds) and b.is_phrase == ("phrases" in kinds)
    assert b.is_bool == ("clauses" in kinds or "phrases" in kinds)
    assert b.is_fscore == ("fscore" in kinds) and b.is_collapse == ("collapse" in kinds)
    assert b.is_bool_tree == ("clause_tree" in kinds) and b.is_script == ("script" in kinds)
    assert (b.agg_spec is not None) == ("aggs" in kinds)
    assert (b.top_hits_spec is not None) == ("top_hits" in kinds)
    assert (b.composite_spec is not None) == ("composite" in kinds)
    assert (b.term_bucket_spec is not None) == ("term_buckets" in kinds)
    if "collapse" in kinds:
        assert b.collapse_shape == (2, 3)


@pytest.mark.parametrize("carried", ["top_hits", "composite", "term_buckets"])
def test_an_aggregation_spec_without_nodes_becomes_null(carried):
    """an aggs.AggPlan of top_hits / composite / term bucket roots alone carries an N.AggSpec of 0 nodes"""
    b, name, args, _ = _prepare(**{carried: True, "aggs": _agg_spec(0)})
    assert name == "slg_batch_prepare_" + carried
    assert args[8] is None and b.agg_spec is None
    b, name, args, _ = _prepare(aggs=_agg_spec(0))  # alone it stays what it is
    assert name == "slg_batch_prepare_aggs" and args[8] is not None and b.agg_spec is not None


def test_the_specs_an_agg_plan_carries_are_taken_from_it():
    class Plan:
        spec = _agg_spec(2)
        top_hits = N.TopHitsSpec()
        composite = None
        term_buckets = None
    b, name, args, _ = _prepare(aggs=Plan)
    assert name == "slg_batch_prepare_top_hits"
    assert args[8] == C.addressof(Plan.spec) and args[9] == C.addressof(Plan.top_hits)
    Plan.top_hits, Plan.composite = None, {"spec": N.CompositeSpec()}
    b, name, args, _ = _prepare(aggs=Plan)
    assert name == "slg_batch_prepare_composite" and args[9] == C.addressof(Plan.composite["spec"])
    Plan.composite, Plan.term_buckets = None, {"spec": N.TermBucketSpec()}
    b, name, args, _ = _prepare(aggs=Plan)
    assert name == "slg_batch_prepare_term_buckets" and args[9] == C.addressof(Plan.term_buckets["spec"])


_CARRIED = ("hybrid", "cursors", "rescore", "clauses", "phrases", "fscore", "collapse", "clause_tree", "script")
REFUSALS = {
    "top_hits": (_CARRIED, "top_hits is built on plain, sorted and aggregation batches only"),
    "composite": (("top_hits",) + _CARRIED, "composite is built on plain, sorted and aggregation batches only"),
    "term_buckets": (("top_hits", "composite") + _CARRIED,
                     "significant_terms and rare_terms are built on plain, sorted and aggregation batches only"),
    "script": (("hybrid", "cursors", "aggs", "rescore", "clauses", "phrases", "collapse", "clause_tree"),
               "script_score is not built on cursor, hybrid, aggregation, rescore, bool, phrase, collapse or matcher "
               "tree batches"),
    "clause_tree": (("hybrid", "cursors", "aggs", "rescore", "clauses", "phrases", "fscore", "collapse"),
                    "a matcher tree is not built on cursor, hybrid, aggregation, rescore, bool, phrase, function_score "
                    "or collapse batches"),
    "collapse": (("hybrid", "aggs", "rescore", "clauses", "phrases", "fscore"),
                 "collapse is not built on hybrid, aggregation, rescore, bool, phrase or function_score batches"),
    "fscore": (("hybrid", "cursors", "aggs", "rescore", "clauses", "phrases"),
               "function_score is not built on cursor, hybrid, aggregation, rescore, bool or phrase batches"),
    "phrases": (("hybrid", "cursors", "aggs", "rescore"),
                "phrases are not built on cursor, hybrid, aggregation or rescore batches"),
    "clauses": (("hybrid", "cursors", "aggs", "rescore"),
                "boolean clauses are not built on cursor, hybrid, aggregation or rescore batches"),
    "rescore": (("hybrid", "cursors", "sort", "aggs"),
                "rescore is not built on sorted, cursor, hybrid or aggregation batches"),
    "aggs": (("hybrid", "cursors"), "aggregations are not built on cursor or hybrid batches"),
}
# two specs of the aggregation family with a third refused argument: the family's lowest member speaks first
DOUBLE = [(("top_hits", "composite", "hybrid"), "top_hits"), (("top_hits", "term_buckets", "rescore"), "top_hits"),
          (("composite", "term_buckets", "script"), "composite"), (("script", "fscore", "clause_tree"), "script"),
          (("clause_tree", "collapse", "fscore"), "clause_tree"), (("rescore", "clauses", "sort"), "clauses")]


def _refused(names, message):
    ix = _Index()
    with pytest.raises(N.SlgError) as e:
        searcher.PreparedBatch(ix, OFFS, TERMS, WEIGHTS, K, STRATEGY, **{n: GIVEN[n]() for n in names})
    assert e.value.code == N.ERR_UNSUPPORTED
    assert e.value.msg == message
    assert not ix._lib.calls and not ix._batches


@pytest.mark.parametrize("kind,other", [(k, o) for k in REFUSALS for o in REFUSALS[k][0]])
def test_every_refused_combination(kind, other):
    _refused((kind, other), REFUSALS[kind][1])


@pytest.mark.parametrize("names,speaker", DOUBLE)
def test_which_kind_refuses_a_doubly_wrong_request(names, speaker):
    _refused(names, REFUSALS[speaker][1])


def test_a_hybrid_batch_takes_no_sort_or_cursor():
    for other in ("sort", "cursors"):
        with pytest.raises(AssertionError):
            _prepare(hybrid=True, **{other: True})
