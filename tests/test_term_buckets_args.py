"""The significant_terms / rare_terms ABI and host mappings, without a device: the new structs against a compiled C
probe, every rejection of slg_batch_prepare_term_buckets that needs no index with its error code, agg_spec's plan and
ValueErrors, and aggs.shape over a hand-made fetch."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def N():
    from searchlite_amd import _native
    return _native


@pytest.fixture(scope="module")
def lib(N):
    return N.load()


def test_structs_match_the_header(N, tmp_path):
    structs = {"slg_term_bucket_node": N.TermBucketNode, "slg_term_bucket_spec": N.TermBucketSpec,
               "slg_term_bucket_node_layout": N.TermBucketNodeLayout, "slg_term_bucket_layout": N.TermBucketLayout}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));\n')
        for f, _ in cls._fields_:
            lines.append(f'  printf(" %zu", offsetof({cname}, {f}));\n')
        lines.append('  printf("\\n");\n')
    lines.append('  printf("limits %u %u %d %d %u\\n", SLG_MAX_TERM_BUCKET_NODES, SLG_MAX_TERM_BUCKET_SIZE, '
                 'SLG_TERMS_SIGNIFICANT, SLG_TERMS_RARE, SLG_MAX_COMPOSITE_SIZE);\n')
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n' +
                   "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]]
           for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    ffi = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    for cname, cls in structs.items():
        size, *offsets = got[cname]
        assert size == C.sizeof(cls), cname
        assert offsets == [getattr(cls, f).offset for f, _ in cls._fields_], cname
        body = re.search(r"pub struct %s \{(.*?)\}" % cname, ffi, re.S).group(1)  # (the Rust mirror: the same fields)
        assert re.findall(r"pub\s+(\w+)\s*:", body) == [f for f, _ in cls._fields_], cname
    assert got["limits"] == [N.MAX_TERM_BUCKET_NODES, N.MAX_TERM_BUCKET_SIZE, N.TERMS_SIGNIFICANT, N.TERMS_RARE,
                             N.MAX_TERM_BUCKET_SIZE]  # (the per-wave set is composite's: the same size cap)
    assert N.term_bucket_cap(N.MAX_TERM_BUCKET_SIZE) == N.composite_cap(N.MAX_COMPOSITE_SIZE)


# ---- rejections without an index ------------------------------------------------------------------------------------
def node(kind=0, field=0, size=10, bound=1, bg=-1, children=()):
    return dict(kind=kind, field=field, size=size, bound=bound, bg=bg, children=children)


def spec_of(N, nodes):
    s = N.TermBucketSpec()
    s.n_nodes = len(nodes)
    for i, nd in enumerate(nodes[:N.MAX_TERM_BUCKET_NODES]):
        t = s.nodes[i]
        t.kind, t.field, t.size, t.doc_count_bound, t.background_filter = nd["kind"], nd["field"], nd["size"], nd["bound"], nd["bg"]
        t.n_children = len(nd["children"])
        for c, fill in enumerate(nd["children"][:N.MAX_AGGS]):
            t.children[c].parent = 99  # (not read)
            fill(t.children[c])
    return s


def prepare(lib, tb, aggs=None, nq=2, k=5):
    offs = np.zeros(nq + 1, np.uint32)
    return lib.slg_batch_prepare_term_buckets(None, nq, offs.ctypes.data, None, None, None, None, None,
                                              None if aggs is None else C.addressof(aggs),
                                              None if tb is None else C.addressof(tb), k, 1)


def fails(lib, N, tb, code, word, aggs=None):
    assert not prepare(lib, tb, aggs)
    assert lib.slg_last_error_code() == getattr(N, code), lib.slg_last_error()
    assert word.encode() in lib.slg_last_error(), lib.slg_last_error()


def kind(k, **kw):
    def fill(n):
        n.kind = k
        for name, v in kw.items():
            setattr(n, name, v)
    return fill


def test_rejections_without_an_index(lib, N):
    S, R = N.TERMS_SIGNIFICANT, N.TERMS_RARE
    fails(lib, N, None, "ERR_INVALID", "term bucket spec is NULL")
    fails(lib, N, spec_of(N, []), "ERR_INVALID", "at least one node")
    fails(lib, N, spec_of(N, [node(), node(kind=2)]), "ERR_INVALID", "node 1: unknown kind")
    fails(lib, N, spec_of(N, [node(kind=R, bg=0)]), "ERR_INVALID", "rare_terms node has no background_filter")
    fails(lib, N, spec_of(N, [node(kind=S, bg=-2)]), "ERR_INVALID", "background_filter < -1")
    fails(lib, N, spec_of(N, [node(kind=R, bg=-2)]), "ERR_INVALID", "background_filter")
    # a child with a defect slg_batch_prepare_aggs rejects as a root
    fails(lib, N, spec_of(N, [node(children=(kind(10),))]), "ERR_INVALID", "unknown kind")
    fails(lib, N, spec_of(N, [node(children=(kind(7),))]), "ERR_INVALID", "unknown kind")
    fails(lib, N, spec_of(N, [node(children=(kind(N.AGG_HISTOGRAM, interval=0.0),))]), "ERR_INVALID", "interval")
    fails(lib, N, spec_of(N, [node(children=(kind(N.AGG_RANGE, n_ranges=0),))]), "ERR_INVALID", "at least one range")
    fails(lib, N, spec_of(N, [node(children=(kind(N.AGG_STATS, has_missing=1, missing=math.nan),))]), "ERR_INVALID", "missing")
    fails(lib, N, spec_of(N, [node(children=(kind(N.AGG_FILTER, filter=-1),))]), "ERR_INVALID", "filter id")
    # unsupported comes behind invalid: both defects, the invalid one is reported
    fails(lib, N, spec_of(N, [node(kind=2, size=0)]), "ERR_INVALID", "unknown kind")
    fails(lib, N, spec_of(N, [node(size=0), node(kind=R, bg=3)]), "ERR_INVALID", "background_filter")
    fails(lib, N, spec_of(N, [node()] * 5), "ERR_UNSUPPORTED", "SLG_MAX_TERM_BUCKET_NODES")
    fails(lib, N, spec_of(N, [node(size=0)]), "ERR_UNSUPPORTED", "size is 0")
    fails(lib, N, spec_of(N, [node(kind=R, size=0)]), "ERR_UNSUPPORTED", "size is 0")
    fails(lib, N, spec_of(N, [node(size=N.MAX_TERM_BUCKET_SIZE + 1)]), "ERR_UNSUPPORTED", "SLG_MAX_TERM_BUCKET_SIZE")
    fails(lib, N, spec_of(N, [node(children=(kind(N.AGG_STATS),) * (N.MAX_AGGS + 1))]), "ERR_UNSUPPORTED", "SLG_MAX_AGGS")
    for k in (N.AGG_CARDINALITY, N.AGG_PERCENTILES, N.AGG_PERCENTILE_RANKS):
        fails(lib, N, spec_of(N, [node(), node(kind=R, children=(kind(N.AGG_STATS), kind(k, n_ranges=1)))]),
              "ERR_UNSUPPORTED", "not built under")
    # the aggregation spec's own checks come first
    bad_aggs = N.AggSpec()
    bad_aggs.n_nodes = 1
    bad_aggs.nodes[0].kind, bad_aggs.nodes[0].parent = 10, -1
    fails(lib, N, None, "ERR_INVALID", "agg node 0", aggs=bad_aggs)
    # a valid spec gets as far as the index
    fails(lib, N, spec_of(N, [node(kind=S, size=N.MAX_TERM_BUCKET_SIZE, bound=0, bg=7,
                                   children=(kind(N.AGG_STATS), kind(N.AGG_TERMS))),
                              node(kind=R, size=1, bound=5)] * 2), "ERR_INVALID", "index is NULL")


def test_other_kinds_refuse_the_calls(lib, N):
    lay = N.TermBucketLayout()
    assert lib.slg_batch_term_buckets_layout(None, C.addressof(lay)) == N.ERR_INVALID
    assert lib.slg_batch_fetch_term_buckets(None, None, None, None, None, None, None, None) == N.ERR_INVALID
    assert lib.slg_search_batch_term_buckets(None, None, 0, None, None, None, None, None, 5, 1, *([None] * 14)) == N.ERR_INVALID


# ---- agg_spec ---------------------------------------------------------------------------------------------------
def fields_of():
    from searchlite_amd import aggs as A
    return {"tag": {"id": 0, "keys": ["b", "a", "é", "ab"]}, "x": {"id": 1}, "dup": {"id": 2, "keys": ["a", "b", "a"]},
            "srt": {"id": 3, "keys": ["a", "b", "c"]}, A.FILTERS: lambda body: {"m": 4}[body["name"]]}


def test_agg_spec_builds_the_plan(N):
    from searchlite_amd import aggs as A
    plan = A.agg_spec({"sig": {"type": "significant_terms", "field": "tag", "size": 7, "min_doc_count": 3,
                               "background_filter": {"name": "m"},
                               "aggs": {"s": {"type": "stats", "field": "x"}, "k": {"type": "terms", "field": "tag"}}},
                       "r": {"type": "rare_terms", "field": "srt", "size": 2},
                       "other": {"type": "stats", "field": "x"}}, fields_of())
    tb = plan.term_buckets
    assert plan.spec.n_nodes == 1 and tb["spec"].n_nodes == 2 and plan.composite is None
    assert [n["name"] for n in tb["nodes"]] == ["r", "sig"]  # (name order, as every root)
    r, s = tb["spec"].nodes[0], tb["spec"].nodes[1]
    assert (r.kind, r.field, r.size, r.doc_count_bound, r.background_filter, r.n_children) == (N.TERMS_RARE, 3, 2, 1, -1, 0)
    assert not r.ord_rank and tb["nodes"][0]["rank"] is None  # (a dictionary in byte order needs no table)
    assert (s.kind, s.field, s.size, s.doc_count_bound, s.background_filter, s.n_children) == \
        (N.TERMS_SIGNIFICANT, 0, 7, 3, 4, 2)
    assert tb["nodes"][1]["rank"].tolist() == [2, 0, 3, 1] and s.ord_rank == tb["nodes"][1]["rank"].ctypes.data
    assert [n["name"] for n in tb["nodes"][1]["children"].nodes] == ["k", "s"]
    assert s.children[0].kind == N.AGG_TERMS and s.children[1].kind == N.AGG_STATS
    # the defaults: min_doc_count 1, max_doc_count 1
    plan = A.agg_spec({"sig": {"type": "significant_terms", "field": "tag", "size": 1},
                       "r": {"type": "rare_terms", "field": "tag", "size": 1, "max_doc_count": 5}}, fields_of())
    assert [n.doc_count_bound for n in plan.term_buckets["spec"].nodes[:2]] == [5, 1]


SIG = {"type": "significant_terms", "field": "tag", "size": 3}
RARE = {"type": "rare_terms", "field": "tag", "size": 3}


@pytest.mark.parametrize("request_, word", [
    ({"s": dict(SIG, sampling={"probability": 0.5})}, "sampling"),
    ({"r": dict(RARE, sampling={"probability": 0.5})}, "sampling"),
    ({"s": {"type": "significant_terms", "field": "tag"}}, "size"),
    ({"r": {"type": "rare_terms", "field": "tag"}}, "size"),
    ({"s": dict(SIG, size=0)}, "size"),
    ({"r": dict(RARE, size=1025)}, "size"),
    ({"p": {"type": "terms", "field": "tag", "aggs": {"s": SIG}}}, "below"),
    ({"p": {"type": "terms", "field": "tag", "aggs": {"r": RARE}}}, "below"),
    ({"s": dict(SIG, aggs={"r": RARE})}, "under"),
    ({"s": dict(SIG, field="x")}, "keyword"),
    ({"s": dict(SIG, field="nope")}, "not registered"),
    ({"s": dict(SIG, field="dup")}, "twice"),
    ({"s": dict(SIG, aggs={"h": {"type": "top_hits", "size": 1}})}, "top_hits"),
    ({"s": dict(SIG, aggs={"n": {"type": "cardinality", "field": "tag"}})}, "cardinality"),
    ({"r": dict(RARE, aggs={"n": {"type": "percentiles", "field": "x"}})}, "percentiles"),
    ({"s": dict(SIG, aggs={"d": {"type": "derivative", "buckets_path": "_count"}})}, "not built"),
    ({"s": dict(SIG, aggs={"k": {"type": "terms", "field": "tag", "aggs": {"s": {"type": "stats", "field": "x"}}}})}, "one level"),
    ({"s": SIG, "c": {"type": "composite", "sources": [{"type": "terms", "name": "t", "field": "tag"}], "size": 3}}, "composite"),
    ({"s": SIG, "h": {"type": "top_hits", "size": 1}}, "top_hits"),
    ({f"s{i}": SIG for i in range(5)}, "more than 4"),
])
def test_agg_spec_value_errors(request_, word):
    from searchlite_amd import aggs as A
    with pytest.raises(ValueError, match=word):
        A.agg_spec(request_, fields_of())


def test_background_filter_needs_the_filter_map():
    from searchlite_amd import aggs as A
    fields = {k: v for k, v in fields_of().items() if k != A.FILTERS}
    with pytest.raises(ValueError, match="background_filter"):
        A.agg_spec({"s": dict(SIG, background_filter={"name": "m"})}, fields)


def test_shape_renders_the_response(N):
    """a hand-made fetch through aggs.shape: ordinals to keys, the score from its bits, children shaped as any
    bucket's, the totals of a significant node only"""
    from searchlite_amd import aggs as A
    plan = A.agg_spec({"sig": dict(SIG, aggs={"s": {"type": "stats", "field": "x"}}), "r": dict(RARE, size=2)}, fields_of())
    lay = dict(rows=5, nodes=[dict(size=2, row_offset=0, count_offset=0, children=[]),
                              dict(size=3, row_offset=2, count_offset=0,
                                   children=[dict(parent_rows=3, rows=1, first_id=0, is_stats=True, is_values=False, offset=0)])])
    stats = np.zeros((1, 3, 1), A.STATS_DTYPE)
    stats[0, 1, 0] = (2, 1.0, 3.0, 4.0)
    bits = np.array([[1.5, 0.25, 0.0]], np.float64).view(np.uint64)
    fetched = dict(nodes=[
        dict(ords=np.array([[3, 0]], np.uint32), doc_counts=np.array([[1, 1]], np.uint64),
             bg_counts=np.zeros((1, 2), np.uint64), score_bits=np.zeros((1, 2), np.uint64), scores=np.zeros((1, 2)),
             n_buckets=np.array([2], np.uint32), doc_count=np.zeros(1, np.uint64), bg_count=np.zeros(1, np.uint64),
             counts=None, children=[]),
        dict(ords=np.array([[2, 1, 0]], np.uint32), doc_counts=np.array([[4, 9, 0]], np.uint64),
             bg_counts=np.array([[5, 40, 0]], np.uint64), score_bits=bits, scores=bits.view(np.float64),
             n_buckets=np.array([2], np.uint32), doc_count=np.array([20], np.uint64), bg_count=np.array([100], np.uint64),
             counts=np.array([[4, 9, 0]], np.uint64), children=[stats])])
    got = A.shape(plan, [], [], 0, term_buckets=(lay, fetched))
    assert got["r"] == {"type": "rare_terms", "buckets": [{"key": "ab", "doc_count": 1}, {"key": "b", "doc_count": 1}]}
    sig = got["sig"]
    assert sig["type"] == "significant_terms" and sig["doc_count"] == 20 and sig["bg_count"] == 100
    assert [(b["key"], b["doc_count"], b["bg_count"], b["score"]) for b in sig["buckets"]] == [("é", 4, 5, 1.5), ("a", 9, 40, 0.25)]
    assert sig["buckets"][1]["aggregations"]["s"] == {"type": "stats", "count": 2, "min": 1.0, "max": 3.0, "sum": 4.0, "avg": 2.0}
    assert sig["buckets"][0]["aggregations"]["s"]["count"] == 0
