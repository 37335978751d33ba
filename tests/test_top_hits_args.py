"""slg_batch_prepare_top_hits / _top_hits_layout / _fetch_top_hits / slg_search_batch_top_hits argument checks that need
no device: the spec is checked before the index is looked at (a NULL index fails with SLG_ERR_INVALID and a message,
before anything touches a GPU); the header, the ctypes binding and the Rust mirror agree on the argument counts and the
structures; searchlite_amd.aggs turns a request's top_hits bodies into the spec and refuses what the device does not
build.

One refusal of the header's list needs the index and is checked on the device (tests/test_gpu_top_hits.py): more than
SLG_MAX_TOP_HITS_CELLS hit cells per query.  The lists of a child are its parent's rows, which for every parent kind
but range and filter follow from the registered column; a range or filter parent cannot reach the limit (16 ranges x 64
hits x 4 nodes = 4096 cells)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {"slg_batch_prepare_top_hits": 12, "slg_batch_top_hits_layout": 2, "slg_batch_fetch_top_hits": 6,
           "slg_search_batch_top_hits": 23}


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


def th_spec(*nodes, n_nodes=None, max_entries=0):
    """nodes: dicts with parent (-1), from (0), size (3), sort = (n_parts, fields, orders)"""
    from searchlite_amd import _native as N
    spec = N.TopHitsSpec()
    spec.n_nodes = len(nodes) if n_nodes is None else n_nodes
    spec.max_entries = max_entries
    for i, nd in enumerate(nodes[:N.MAX_TOP_HITS_NODES]):
        t = spec.nodes[i]
        t.parent, t.from_, t.size = nd.get("parent", -1), nd.get("from", 0), nd.get("size", 3)
        n_parts, fields, orders = nd.get("sort", (0, [], []))
        t.sort.n_parts = n_parts
        for j, (f, o) in enumerate(zip(fields, orders)):
            t.sort.field[j], t.sort.order[j] = f, o
    return spec


def agg_spec(*nodes):
    """nodes: (kind, parent) of an aggregation spec that passes its own checks"""
    from searchlite_amd import _native as N
    spec = N.AggSpec()
    spec.n_nodes = len(nodes)
    for i, (kind, parent) in enumerate(nodes):
        n = spec.nodes[i]
        n.kind, n.parent, n.field = kind, parent, 0
        if kind == N.AGG_HISTOGRAM:
            n.interval = 1.0
        if kind == N.AGG_RANGE:
            n.n_ranges = 1
        if kind == N.AGG_DATE_HISTOGRAM:
            n.calendar_unit = N.DATE_DAY
    return spec


def prepare(lib, th, aggs=None, nq=2, k=11):
    offs = np.zeros(nq + 1, np.uint32)
    return lib.slg_batch_prepare_top_hits(None, nq, offs.ctypes.data, None, None, None, None, None,
                                          None if aggs is None else C.addressof(aggs),
                                          None if th is None else C.addressof(th), k, 1)


def rejected(lib, th, code, word, aggs=None, **kw):
    from searchlite_amd import _native as N
    assert prepare(lib, th, aggs, **kw) is None
    assert lib.slg_last_error_code() == getattr(N, code), lib.slg_last_error()
    assert word.encode() in lib.slg_last_error(), lib.slg_last_error()


def passes(lib, th, aggs=None, **kw):
    """a spec that passes every index-free check: the index is looked at next"""
    rejected(lib, th, "ERR_INVALID", "index is NULL", aggs, **kw)


def _n_args(text, pattern):
    m = re.search(pattern, text, re.S)
    assert m, pattern
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(EXPORTS))
def test_export_and_argument_counts(lib, name):
    assert hasattr(lib, name), f"{name} is not exported"
    assert len(getattr(lib, name).argtypes) == EXPORTS[name]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "searchlite_gpu.h")).read(), flags=re.S)
    assert _n_args(header, r"\b%s\s*\((.*?)\)\s*;" % name) == EXPORTS[name]
    rs = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    assert _n_args(rs, r"pub fn %s\((.*?)\)\s*->" % name) == EXPORTS[name]


def test_struct_layouts_match_the_header_and_the_rust_mirror(tmp_path):
    from searchlite_amd import _native as N
    structs = {"slg_top_hits_node": (N.TopHitsNode, {"from_": "from"}), "slg_top_hits_spec": (N.TopHitsSpec, {}),
               "slg_top_hits_layout": (N.TopHitsLayout, {})}
    lines = []
    for cname, (cls, rename) in structs.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));\n')
        for f, _ in cls._fields_:
            lines.append(f'  printf(" %zu", offsetof({cname}, {rename.get(f, f)}));\n')
        lines.append('  printf("\\n");\n')
    lines.append('  printf("limits %u %u %u %u %zu\\n", SLG_MAX_TOP_HITS_NODES, SLG_MAX_TOP_HITS, SLG_MAX_TOP_HITS_CELLS,\n'
                 '         SLG_MAX_TOP_HITS_ENTRIES, sizeof(slg_agg_node));\n')
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n' +
                   "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    ffi = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    for cname, (cls, rename) in structs.items():
        size, *offsets = got[cname]
        assert size == C.sizeof(cls), cname
        assert offsets == [getattr(cls, f).offset for f, _ in cls._fields_], cname
        body = re.search(r"pub struct %s \{(.*?)\}" % cname, ffi, re.S).group(1)
        assert re.findall(r"pub\s+(\w+)\s*:", body) == [rename.get(f, f) for f, _ in cls._fields_], cname
    assert got["limits"] == [N.MAX_TOP_HITS_NODES, N.MAX_TOP_HITS, N.MAX_TOP_HITS_CELLS, N.MAX_TOP_HITS_ENTRIES, 368]
    assert got["limits"][:4] == [4, 64, 65536, 1 << 19]  # (slg_agg_node did not grow: the spec travels beside it)
    for line in ("pub const SLG_MAX_TOP_HITS_NODES: usize = 4;", "pub const SLG_MAX_TOP_HITS: u32 = 64;",
                 "pub const SLG_MAX_TOP_HITS_CELLS: u32 = 65536;", "pub const SLG_MAX_TOP_HITS_ENTRIES: u32 = 1 << 19;"):
        assert line in ffi, line


def test_null_spec_null_index_and_node_count(lib):
    from searchlite_amd import _native as N
    rejected(lib, None, "ERR_INVALID", "top_hits spec is NULL")
    rejected(lib, th_spec(), "ERR_INVALID", "at least one node")
    passes(lib, th_spec({}))
    passes(lib, th_spec({}), nq=0)
    passes(lib, th_spec({}), k=0)
    passes(lib, th_spec(*[{}] * N.MAX_TOP_HITS_NODES))
    rejected(lib, th_spec(*[{}] * N.MAX_TOP_HITS_NODES, n_nodes=N.MAX_TOP_HITS_NODES + 1), "ERR_UNSUPPORTED",
             "SLG_MAX_TOP_HITS_NODES")
    passes(lib, th_spec({}, max_entries=17))
    # the aggregation spec's own checks come first
    bad = agg_spec((N.AGG_HISTOGRAM, -1))
    bad.nodes[0].interval = 0.0
    rejected(lib, th_spec({"parent": 0}), "ERR_INVALID", "interval", bad)


def test_parents(lib):
    from searchlite_amd import _native as N
    buckets = (N.AGG_TERMS, N.AGG_HISTOGRAM, N.AGG_RANGE, N.AGG_DATE_HISTOGRAM, N.AGG_FILTER)
    for kind in buckets:
        passes(lib, th_spec({"parent": 0}, {}), agg_spec((kind, -1)))
    rejected(lib, th_spec({"parent": 0}), "ERR_INVALID", "needs an aggregation spec")  # aggs NULL with a child node
    passes(lib, th_spec({}, {}))  # roots alone need none
    two = agg_spec((N.AGG_TERMS, -1), (N.AGG_STATS, 0))
    rejected(lib, th_spec({"parent": 2}), "ERR_INVALID", "not a node", two)
    rejected(lib, th_spec({"parent": -2}), "ERR_INVALID", "not a node", two)
    rejected(lib, th_spec({"parent": 1}), "ERR_INVALID", "not a bucket node", two)
    for kind in (N.AGG_STATS, N.AGG_CARDINALITY):
        rejected(lib, th_spec({"parent": 0}), "ERR_INVALID", "not a bucket node", agg_spec((kind, -1)))
    # a parent that is itself a child: a third level
    deep = agg_spec((N.AGG_TERMS, -1), (N.AGG_HISTOGRAM, 0))
    rejected(lib, th_spec({"parent": 1}), "ERR_UNSUPPORTED", "third level", deep)
    passes(lib, th_spec({"parent": 0}, {"parent": 0}, {}), deep)  # two nodes under one parent, and a root
    # an invalid argument is reported before an unsupported one
    rejected(lib, th_spec({"parent": 1}, {"parent": 7}), "ERR_INVALID", "not a node", deep)


def test_size_and_from(lib):
    from searchlite_amd import _native as N
    m = N.MAX_TOP_HITS
    rejected(lib, th_spec({"size": 0}), "ERR_UNSUPPORTED", "size is 0")
    passes(lib, th_spec({"size": m}))
    passes(lib, th_spec({"from": m - 1, "size": 1}))
    rejected(lib, th_spec({"size": m + 1}), "ERR_UNSUPPORTED", "SLG_MAX_TOP_HITS")
    rejected(lib, th_spec({"from": m, "size": 1}), "ERR_UNSUPPORTED", "SLG_MAX_TOP_HITS")
    rejected(lib, th_spec({"from": 0xFFFFFFFF, "size": 2}), "ERR_UNSUPPORTED", "SLG_MAX_TOP_HITS")
    rejected(lib, th_spec({}, {"size": 0}), "ERR_UNSUPPORTED", "node 1")


def test_sorts(lib):
    from searchlite_amd import _native as N
    n = N.MAX_SORT_PARTS
    passes(lib, th_spec({"sort": (n, [0, 1, 2, -1], [0, 1, 0, 1])}))
    passes(lib, th_spec({"sort": (0, [], [])}))  # `_score` desc
    rejected(lib, th_spec({"sort": (n + 1, [0] * n, [0] * n)}), "ERR_UNSUPPORTED", "SLG_MAX_SORT_PARTS")
    rejected(lib, th_spec({"sort": (2, [0, 0], [0, 2])}), "ERR_INVALID", "sort order")
    rejected(lib, th_spec({"sort": (1, [0], [-1])}), "ERR_INVALID", "sort order")
    rejected(lib, th_spec({"sort": (2, [0, -2], [0, 0])}), "ERR_INVALID", "sort field")
    # an invalid argument is reported before an unsupported one
    rejected(lib, th_spec({"sort": (n + 1, [0] * n, [0, 0, 7, 0])}), "ERR_INVALID", "sort order")
    rejected(lib, th_spec({"size": 0}, {"sort": (1, [0], [5])}), "ERR_INVALID", "sort order")


def test_other_entries_null_arguments(lib):
    from searchlite_amd import _native as N
    assert lib.slg_batch_fetch_top_hits(*[None] * 6) == N.ERR_INVALID
    assert b"batch" in lib.slg_last_error()
    assert lib.slg_batch_top_hits_layout(None, None) == N.ERR_INVALID
    assert b"batch" in lib.slg_last_error()
    sp = th_spec({})
    assert lib.slg_search_batch_top_hits(None, None, 0, None, None, None, None, C.addressof(sp), 11, 1,
                                         *[None] * 13) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error()


def test_python_layer_refuses_the_kinds_top_hits_is_not_built_on():
    """the library's other prepare calls take no top_hits spec: PreparedBatch refuses the combination itself, before it
    touches the index"""
    from searchlite_amd import _native as N
    from searchlite_amd.searcher import PreparedBatch

    class NoIndex:
        _lib = None
    offs = np.zeros(2, np.uint32)
    for kind in ("hybrid", "cursors", "rescore", "clauses", "phrases", "fscore", "collapse", "clause_tree", "script"):
        with pytest.raises(N.SlgError) as ei:
            PreparedBatch(NoIndex(), offs, np.zeros(0, np.uint32), np.zeros(0, np.float32), 11, 1,
                          top_hits=th_spec({}), **{kind: True if kind == "hybrid" else [None] if kind == "cursors" else {}})
        assert ei.value.code == N.ERR_UNSUPPORTED and "top_hits" in ei.value.msg
    # a scan batch takes an aggregation plan, but not one with top_hits nodes: nothing is dropped silently
    from searchlite_amd import aggs as A
    from searchlite_amd.searcher import ScanBatch
    plan = A.agg_spec({"newest": {"type": "top_hits", "size": 5}}, {})
    with pytest.raises(N.SlgError) as ei:
        ScanBatch(NoIndex(), [{"match_all": {}}], 11, aggs=plan)
    assert ei.value.code == N.ERR_UNSUPPORTED and "scan" in ei.value.msg


FIELDS ={"kw": {"id": 3, "keys": ["a", "b"]}, "x": {"id": 4, "sort_id": 9}, "y": {"id": 5, "sort_id": 2},
          "plain": {"id": 6}}


def test_agg_plan_contents():
    from searchlite_amd import _native as N
    from searchlite_amd import aggs as A
    request = {"by_kw": {"type": "terms", "field": "kw",
                         "aggs": {"s": {"type": "stats", "field": "x"},
                                  "best": {"type": "top_hits", "size": 3, "from": 2, "fields": ["kw"],
                                           "sort": [{"field": "x", "order": "desc"}, {"field": "_score"},
                                                    {"field": "y"}]}}},
               "newest": {"type": "top_hits", "size": 5}}
    plan = A.agg_spec(request, FIELDS)
    # .spec and .nodes keep their content: the bucket node and its stats child, nothing of the top_hits nodes
    assert plan.spec.n_nodes == 2 and [nd["name"] for nd in plan.nodes] == ["by_kw", "s"]
    assert [int(plan.spec.nodes[i].kind) for i in range(2)] == [N.AGG_TERMS, N.AGG_STATS]
    assert plan.top_hits_nodes == [
        {"name": "best", "parent": 0, "from": 2, "size": 3, "sort": [(9, "desc"), ("_score", "desc"), (2, "asc")]},
        {"name": "newest", "parent": -1, "from": 0, "size": 5, "sort": []}]
    th = plan.top_hits
    assert th.n_nodes == 2 and th.max_entries == 0
    a, b = th.nodes[0], th.nodes[1]
    assert (a.parent, a.from_, a.size, a.sort.n_parts) == (0, 2, 3, 3)
    assert list(a.sort.field)[:3] == [9, N.SORT_SCORE, 2] and list(a.sort.order)[:3] == [N.ORDER_DESC, N.ORDER_DESC, N.ORDER_ASC]
    assert (b.parent, b.from_, b.size, b.sort.n_parts) == (-1, 0, 5, 0)
    # a request without top_hits: as before
    plain = A.agg_spec({"by_kw": {"type": "terms", "field": "kw"}}, FIELDS)
    assert plain.top_hits is None and plain.top_hits_nodes == [] and plain.spec.n_nodes == 1
    # roots alone: no aggregation node at all
    roots = A.agg_spec({"newest": {"type": "top_hits", "size": 5}}, FIELDS)
    assert roots.spec.n_nodes == 0 and roots.nodes == [] and roots.top_hits.n_nodes == 1


@pytest.mark.parametrize("body,word", [
    ({"type": "top_hits", "size": 0}, "size 0"),
    ({"type": "top_hits", "size": 65}, "from + size"),
    ({"type": "top_hits", "size": 1, "from": 64}, "from + size"),
    ({"type": "top_hits", "size": 3, "sort": [{"field": "kw"}]}, "keyword sort part"),
    ({"type": "top_hits", "size": 3, "sort": [{"field": "plain"}]}, "without a sort column"),
    ({"type": "top_hits", "size": 3, "sort": [{"field": "nope"}]}, "not registered"),
    ({"type": "top_hits", "size": 3, "sort": [{"field": "x", "order": "up"}]}, "sort order"),
    ({"type": "top_hits", "size": 3, "sort": [{"field": "x"}] * 5}, "sort parts"),
    ({"type": "top_hits", "size": 3, "aggs": {"s": {"type": "stats", "field": "x"}}}, "no children"),
])
def test_agg_spec_refuses_what_the_device_does_not_build(body, word):
    from searchlite_amd import aggs as A
    for request in ({"h": body}, {"t": {"type": "terms", "field": "kw", "aggs": {"h": body}}}):
        with pytest.raises(ValueError, match=re.escape(word)):
            A.agg_spec(request, FIELDS)


def test_agg_spec_refuses_a_fifth_node_and_a_missing_size_and_takes_max_entries():
    from searchlite_amd import _native as N
    from searchlite_amd import aggs as A
    hits = {"type": "top_hits", "size": 3}
    four = {f"h{i}": hits for i in range(N.MAX_TOP_HITS_NODES)}
    assert A.agg_spec(four, FIELDS).top_hits.n_nodes == N.MAX_TOP_HITS_NODES
    with pytest.raises(ValueError, match="more than 4 top_hits"):
        A.agg_spec(dict(four, one_more=hits), FIELDS)
    with pytest.raises(ValueError, match="requires `size`"):
        A.agg_spec({"h": {"type": "top_hits"}}, FIELDS)
    assert A.agg_spec(four, FIELDS, top_hits_max_entries=1234).top_hits.max_entries == 1234
    assert A.agg_spec(four, FIELDS).top_hits.max_entries == 0  # the library's default capacity


def test_agg_spec_refuses_a_third_level_and_a_metric_parent():
    from searchlite_amd import aggs as A
    hits = {"type": "top_hits", "size": 3}
    deep = {"t": {"type": "terms", "field": "kw", "aggs": {"h": {"type": "histogram", "field": "x", "interval": 1.0,
                                                                 "aggs": {"best": hits}}}}}
    with pytest.raises(ValueError, match="two levels"):
        A.agg_spec(deep, FIELDS)
    with pytest.raises(ValueError, match="two levels"):
        A.agg_spec({"s": {"type": "stats", "field": "x", "aggs": {"best": hits}}}, FIELDS)


def test_shape_emits_top_hits_in_the_bucket_and_at_the_root():
    from searchlite_amd import aggs as A
    request = {"by_kw": {"type": "terms", "field": "kw", "aggs": {"best": {"type": "top_hits", "size": 2}}},
               "all": {"type": "top_hits", "size": 2, "from": 1}}
    plan = A.agg_spec(request, FIELDS)
    layout = [dict(parent_rows=1, rows=2, first_id=0, is_stats=False, is_values=False, offset=0)]
    tables = [np.array([[[3, 0]]], np.uint64)]
    z = lambda *shape: np.zeros(shape, np.uint32)
    best = dict(doc=z(1, 2, 2), seg=z(1, 2, 2), score=np.zeros((1, 2, 2), np.float32), count=z(1, 2))
    best["doc"][0, 0], best["seg"][0, 0], best["score"][0, 0], best["count"][0, 0] = [7, 5], [1, 0], [2.5, 1.5], 2
    root = dict(doc=z(1, 1, 2), seg=z(1, 1, 2), score=np.zeros((1, 1, 2), np.float32), count=z(1, 1))
    root["doc"][0, 0, 0], root["score"][0, 0, 0], root["count"][0, 0] = 5, 1.5, 1
    assert [th["name"] for th in plan.top_hits_nodes] == ["all", "best"]  # (the walk is in name order)
    hits = dict(status=z(1), nodes=[root, best])
    got = A.shape(plan, layout, tables, 0, hits, matched=np.array([3], np.uint64))
    assert got == {
        "by_kw": {"type": "terms", "buckets": [{"key": "a", "doc_count": 3, "aggregations": {"best": {
            "type": "top_hits", "total": 3, "hits": [{"segment": 1, "doc": 7, "score": 2.5},
                                                     {"segment": 0, "doc": 5, "score": 1.5}]}}}]},
        "all": {"type": "top_hits", "total": 3, "hits": [{"segment": 0, "doc": 5, "score": 1.5}]}}
    # without the arrays: the response of the other kinds, as before
    assert A.shape(plan, layout, tables, 0) == {"by_kw": {"type": "terms", "buckets": [{"key": "a", "doc_count": 3}]}}
    hits["status"][0] = 1
    with pytest.raises(ValueError, match="CPU path"):
        A.shape(plan, layout, tables, 0, hits, matched=np.array([3], np.uint64))
