"""slg_batch_prepare_bool_tree / slg_search_batch_bool_tree without a device: every refusal of the spec with its
code (the spec is checked before the index is looked at; a NULL index then fails with SLG_ERR_INVALID), the term
ids, filter ids, row order and node masks of the planned tables through the host planner (plan_bool_tree: pure host
code), the spec's layout against the header and both mirrors, and the three-valued rule the kernel runs after every
step of a row (slg::booltree_eval through the plan C API): a decided root equals the root of every completion of the
open leaves, and with every leaf known the root is decided."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from searchlite_amd import booltree as BT
from tests import booltree_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {"slg_batch_prepare_bool_tree": 11, "slg_search_batch_bool_tree": 17}
MUST, SHOULD, MUST_NOT = R.MUST, R.SHOULD, R.MUST_NOT
T = lambda *ids: {"term": list(ids)}


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


# bool{must: [t0], should: [dis_max{[t1, t2], t3}], must_not: [t4], filter: [0]}, walked must, must_not, filter,
# should: leaf 0 = {t0}, leaf 1 = {t4}, leaf 2 = {t1, t2}, leaf 3 = {t3}, leaf 4 the filter; node 0 the dis_max,
# node 1 the root
DEFAULT = {"bool": {"must": [T(0)], "should": [{"dis_max": [T(1, 2), T(3)]}], "must_not": [T(4)], "filter": [0]}}


def spec_of(queries=None, n_segs=1, **over):
    """the spec of the nested descriptions `queries` (default: DEFAULT twice); over: fields replaced (None: a NULL
    pointer) -> (N.BoolTreeSpec, the arrays it points into)"""
    from searchlite_amd import _native as N
    tree = BT.compile_matchers([DEFAULT, DEFAULT] if queries is None else queries, n_segs)
    a = {("c_term_ids" if n == "c_terms" else n): v for n, v in tree.items()}
    a.update(over)
    a = {n: None if v is None else np.ascontiguousarray(v) for n, v in a.items()}
    return N.BoolTreeSpec(*[None if a[n] is None else a[n].ctypes.data for n, _ in N.BoolTreeSpec._fields_]), a


def prepare(lib, spec, nq=2, k=11, plans=None):
    offs = np.zeros(nq + 1, np.uint32)
    return lib.slg_batch_prepare_bool_tree(None, nq, offs.ctypes.data, None, None,
                                           None if plans is None else C.addressof(plans), None, None,
                                           None if spec is None else C.addressof(spec), k, 1)


def rejected(lib, spec, code, word, **kw):
    from searchlite_amd import _native as N
    sp, keep = spec if spec is not None else (None, None)
    assert prepare(lib, sp, **kw) is None
    assert lib.slg_last_error_code() == getattr(N, code), lib.slg_last_error()
    assert word.encode() in lib.slg_last_error(), lib.slg_last_error()


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


def test_spec_layout_matches_the_header_and_the_rust_mirror(tmp_path):
    import subprocess
    from searchlite_amd import _native as N
    fields = [n for n, _ in N.BoolTreeSpec._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n'
                   '  printf("%zu %u %u %u", sizeof(slg_bool_tree_spec), SLG_MAX_BOOL_TREE_LEAVES, SLG_MAX_BOOL_TREE_NODES,\n'
                   '         SLG_MAX_BOOL_TERMS);\n' +
                   "".join(f'  printf(" %zu", offsetof(slg_bool_tree_spec, {f}));\n' for f in fields) +
                   '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, max_l, max_n, max_t, *offsets = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(N.BoolTreeSpec) and len(fields) == 11
    assert offsets == [getattr(N.BoolTreeSpec, f).offset for f in fields]
    assert max_l == N.MAX_BOOL_TREE_LEAVES == 32 and max_n == N.MAX_BOOL_TREE_NODES == 32 and max_t == N.MAX_BOOL_TERMS
    ffi = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    body = re.search(r"pub struct slg_bool_tree_spec \{(.*?)\}", ffi, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", body) == fields
    for name in ("SLG_MAX_BOOL_TREE_LEAVES", "SLG_MAX_BOOL_TREE_NODES"):
        assert re.search(r"pub const %s: \w+ = 32;" % name, ffi), name


def test_null_spec_and_null_index(lib):
    rejected(lib, None, "ERR_INVALID", "bool tree spec is NULL")
    rejected(lib, spec_of(), "ERR_INVALID", "index is NULL")  # a valid spec: the index is looked at next
    rejected(lib, spec_of([]), "ERR_INVALID", "index is NULL", nq=0)
    rejected(lib, spec_of([None, None]), "ERR_INVALID", "index is NULL")  # no query has a matcher
    rejected(lib, spec_of([None, "match_all"]), "ERR_INVALID", "index is NULL")  # a node without a leaf
    rejected(lib, spec_of([{"dis_max": []}, T(0)]), "ERR_INVALID", "index is NULL")


@pytest.mark.parametrize("name", ["c_offsets", "g_offsets", "f_offsets", "n_offsets", "c_term_ids", "c_group",
                                  "f_filter", "n_min_should", "e_offsets", "e_child", "e_kind"])
def test_null_arrays(lib, name):
    rejected(lib, spec_of(**{name: None}), "ERR_INVALID", name)


def test_arrays_nothing_points_into_may_be_null(lib):
    rejected(lib, spec_of([None, None], c_term_ids=None, c_group=None, f_filter=None, n_min_should=None,
                          e_offsets=None, e_child=None, e_kind=None), "ERR_INVALID", "index is NULL")
    rejected(lib, spec_of(["match_all", None], c_term_ids=None, c_group=None, f_filter=None, e_child=None,
                          e_kind=None), "ERR_INVALID", "index is NULL")


def test_offsets_that_decrease(lib):
    rejected(lib, spec_of(c_offsets=np.array([0, 6, 5], np.uint32)), "ERR_INVALID", "c_offsets not monotone")
    rejected(lib, spec_of(g_offsets=np.array([0, 4, 3], np.uint32)), "ERR_INVALID", "g_offsets not monotone")
    rejected(lib, spec_of(f_offsets=np.array([0, 2, 1], np.uint32)), "ERR_INVALID", "f_offsets not monotone")
    rejected(lib, spec_of(n_offsets=np.array([0, 4, 2], np.uint32)), "ERR_INVALID", "n_offsets not monotone")
    rejected(lib, spec_of(e_offsets=np.array([0, 2, 6, 5, 12], np.uint32)), "ERR_INVALID", "e_offsets not monotone")


def test_bad_groups(lib):
    good = np.array([0, 1, 2, 2, 3] * 2, np.uint32)
    rejected(lib, spec_of(c_group=good), "ERR_INVALID", "index is NULL")
    rejected(lib, spec_of(c_group=np.array([0, 1, 0, 2, 3] + [0, 1, 2, 2, 3], np.uint32)), "ERR_INVALID", "decreases or skips")
    rejected(lib, spec_of(c_group=np.array([0, 0, 2, 2, 3] + [0, 1, 2, 2, 3], np.uint32)), "ERR_INVALID", "decreases or skips")
    rejected(lib, spec_of(c_group=np.array([0, 1, 2, 3, 4] + [0, 1, 2, 2, 3], np.uint32)), "ERR_INVALID", "does not have")
    rejected(lib, spec_of(c_group=np.array([0, 1, 2, 2, 2] + [0, 1, 2, 2, 3], np.uint32)), "ERR_INVALID", "group without a term")


def edges(**over):
    """DEFAULT's edges — node 0: (2 S) (3 S); node 1 = the root: (0 M) (1 MN) (4 M) (5 S) — with replacements"""
    child = np.array([2, 3, 0, 1, 4, 5] * 2, np.uint32)
    kind = np.array([SHOULD, SHOULD, MUST, MUST_NOT, MUST, SHOULD] * 2, np.int32)
    for i, v in over.get("child", {}).items():
        child[i] = v
    for i, v in over.get("kind", {}).items():
        kind[i] = v
    return dict(e_child=child, e_kind=kind)


def test_default_edges_are_what_the_cases_below_edit():
    sp, a = spec_of()
    want = edges()
    assert a["e_child"].tolist() == want["e_child"].tolist() and a["e_kind"].tolist() == want["e_kind"].tolist()
    assert a["e_offsets"].tolist() == [0, 2, 6, 8, 12] and a["n_min_should"].tolist() == [1, 0, 1, 0]


@pytest.mark.parametrize("kind", [-1, 3, 100])
def test_unknown_kind(lib, kind):
    rejected(lib, spec_of(**edges(kind={9: kind})), "ERR_INVALID", "unknown child kind")


def test_child_index_not_below_its_node(lib):
    rejected(lib, spec_of(**edges(child={0: 5})), "ERR_INVALID", "not below its node")    # node 0 names itself
    rejected(lib, spec_of(**edges(child={1: 6})), "ERR_INVALID", "not below its node")    # node 0 names the root
    rejected(lib, spec_of(**edges(child={11: 6})), "ERR_INVALID", "not below its node")   # the root names itself
    rejected(lib, spec_of(**edges(child={11: 77})), "ERR_INVALID", "not below its node")


def test_unreferenced_values_and_leaves_without_a_node(lib):
    rejected(lib, spec_of(**edges(child={1: 2})), "ERR_INVALID", "a leaf that no node references")  # leaf 3 dropped
    rejected(lib, spec_of(**edges(child={5: 4})), "ERR_INVALID", "a node other than the root that no node references")
    rejected(lib, spec_of(n_offsets=np.array([0, 0, 2], np.uint32)), "ERR_INVALID", "leaves but no node")
    rejected(lib, spec_of(f_filter=np.array([0, -1], np.int32)), "ERR_INVALID", "unknown filter id")


def test_min_match_in_the_plans(lib):
    from searchlite_amd import _native as N
    for mm, ok in (([0, 1], True), ([1, 2], False), ([5, 0], False)):
        arr = np.array(mm, np.uint32)
        plans = N.ScorePlans()
        plans.q_min_match = arr.ctypes.data
        rejected(lib, spec_of(), "ERR_INVALID", "index is NULL" if ok else "q_min_match", plans=plans)


def chain(n):
    """n nodes, each holding a leaf and the node before it: n leaves, the root is node n - 1"""
    d = {"bool": {"must": [T(0)]}}
    for i in range(1, n):
        d = {"bool": {"should": [T(i % 7), d], "minimum_should_match": 1}} if i % 2 else {"bool": {"must": [T(i % 7)], "must_not": [d]}}
    return d


def test_limits(lib):
    wide = lambda n, per=1: {"bool": {"should": [T(*range(g, g + per)) for g in range(n)]}}
    rejected(lib, spec_of([wide(32, 2), chain(32)]), "ERR_INVALID", "index is NULL")  # 32 leaves / 64 terms; 32 nodes
    rejected(lib, spec_of([wide(33), None]), "ERR_UNSUPPORTED", "SLG_MAX_BOOL_TREE_LEAVES")
    rejected(lib, spec_of([{"bool": {"should": [T(g) for g in range(31)], "filter": [3, 4]}}, None]), "ERR_UNSUPPORTED",
             "SLG_MAX_BOOL_TREE_LEAVES")  # filter leaves count
    rejected(lib, spec_of([None, chain(33)]), "ERR_UNSUPPORTED", "SLG_MAX_BOOL_TREE")
    rejected(lib, spec_of([None, {"bool": {"should": ["match_all"] * 32}}]), "ERR_UNSUPPORTED", "SLG_MAX_BOOL_TREE_NODES")
    rejected(lib, spec_of([None, {"bool": {"must": [T(*range(65))]}}]), "ERR_UNSUPPORTED", "SLG_MAX_BOOL_TERMS")
    twice = dict(e_offsets=np.array([0, 3, 7, 9, 13], np.uint32),  # node 0 of query 0: leaf 3 twice
                 e_child=np.array([2, 3, 3, 0, 1, 4, 5] + [2, 3, 0, 1, 4, 5], np.uint32),
                 e_kind=np.array([SHOULD, SHOULD, SHOULD, MUST, MUST_NOT, MUST, SHOULD] + [SHOULD, SHOULD, MUST, MUST_NOT, MUST, SHOULD], np.int32))
    rejected(lib, spec_of(**twice), "ERR_UNSUPPORTED", "same child twice")
    # an invalid argument is reported before an unsupported one, also in a later query
    sp = spec_of([wide(33), DEFAULT])
    kind = sp[1]["e_kind"].copy()
    kind[-1] = 9
    rejected(lib, spec_of([wide(33), DEFAULT], e_kind=kind), "ERR_INVALID", "unknown child kind")
    # min_should above the number of SHOULD children is valid (it matches nothing)
    rejected(lib, spec_of([{"bool": {"should": [T(0)], "minimum_should_match": 9}}] * 2), "ERR_INVALID", "index is NULL")


def test_one_call_form_null_arguments(lib):
    from searchlite_amd import _native as N
    sp, keep = spec_of()
    args = (None, None, None, None, None, None)
    assert lib.slg_search_batch_bool_tree(None, 0, None, None, None, None, None, None, C.addressof(sp), 11, 1, *args) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error()
    assert lib.slg_search_batch_bool_tree(None, 0, None, None, None, None, None, None, None, 11, 1, *args) == N.ERR_INVALID
    assert b"bool tree spec is NULL" in lib.slg_last_error()


# ---- the host planner: term and filter ids against the index, and the tables the kernel reads ----
class Seg(C.Structure):
    _fields_ = [("n_docs", C.c_uint32), ("n_terms", C.c_uint32), ("term_offsets", C.c_void_p), ("champ", C.c_void_p)]


def plan_lib():
    from searchlite_amd import build
    L = C.CDLL(build.build_plan_lib())
    L.slgp_plan_bool_tree.restype = C.c_int
    L.slgp_booltree_eval.restype = None
    return L


def plan_tree(queries, seg_offsets, filter_live=(1, 1), plans=None):
    """-> (code, message, tables) of slgplan::plan_bool_tree over segments with the given term_offsets; tables:
    queries [nq, 8], nodes [(must, must_not, should, min_should)], terms [(off, df, group)], filters (addresses),
    filt_rows"""
    L = plan_lib()
    offs = [np.asarray(o, np.uint64) for o in seg_offsets]
    segs = (Seg * len(offs))(*[Seg(100, len(o) - 1, o.ctypes.data, None) for o in offs])
    sp, keep = spec_of(queries, len(offs))
    nq = len(queries)
    live = np.array(filter_live, np.int8)
    qw, nw, tw = np.zeros((max(nq, 1), 8), np.uint32), np.zeros((256, 8), np.uint32), np.zeros((4096, 4), np.uint32)
    fw, rw, counts = np.zeros(256, np.uint64), np.zeros(256, np.uint32), np.zeros(4, np.uint32)
    err = C.create_string_buffer(256)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    rc = L.slgp_plan_bool_tree(segs, len(offs), vp(live), len(live), nq, C.byref(sp),
                               None if plans is None else C.byref(plans), vp(qw), vp(nw), 256, vp(tw), 4096, vp(fw), 256,
                               vp(rw), 256, vp(counts), err, 256)
    n_nodes, n_terms, n_filters, n_rows = (int(x) for x in counts)
    u64 = lambda lo, hi: int(lo) | (int(hi) << 32)
    nodes = [(u64(w[0], w[1]), u64(w[2], w[3]), u64(w[4], w[5]), int(w[6])) for w in nw[:n_nodes]]
    terms = [(u64(lo, hi), int(df), int(g)) for lo, hi, df, g in tw[:n_terms]]
    return rc, err.value.decode(), dict(queries=qw[:nq].tolist(), nodes=nodes, terms=terms,
                                        filters=fw[:n_filters].tolist(), filt_rows=rw[:n_rows].tolist())


def test_term_and_filter_ids_against_the_index():
    from searchlite_amd import _native as N
    offs = [[0, 3, 3, 10], [0, 5]]  # 3 terms, 1 term
    q = lambda t: [{"bool": {"must": [{"dis_max": [T(t)]}]}}]
    assert plan_tree(q((2, 0)), offs)[0] == N.OK
    assert plan_tree(q((2, N.NO_TERM)), offs)[0] == N.OK
    for bad in ((3, 0), (0, 1), (0xFFFFFFFE, 0)):
        rc, msg, _ = plan_tree(q(bad), offs)
        assert rc == N.ERR_INVALID and "term id out of range" in msg, (bad, rc, msg)
    f = lambda i: [{"bool": {"must": [T(0)], "filter": [i]}}]
    assert plan_tree(f(1), offs)[0] == N.OK
    for bad, live in ((2, (1, 1)), (1, (1, 0)), (0, ())):
        rc, msg, _ = plan_tree(f(bad), offs, filter_live=live)
        assert rc == N.ERR_INVALID and "unknown filter id" in msg, (bad, rc, msg)


END = 0x100  # BoolTerm::group: the last term of its leaf


def test_tables_of_plan_bool_tree():
    """node masks over the 64 value bits; the row: first the terms of the leaves that reach the root over MUST /
    MUST_NOT edges only, then the others, each class in the caller's order, a leaf's terms side by side and the last
    one marked; offsets in the padded layout (+ 64 per term); an absent term and an empty list have df 0; a query
    without a matcher has no tables; the filter table holds each used filter once, in order of first use"""
    from searchlite_amd import _native as N
    offs = [[0, 3, 3, 10], [0, 5, 9]]
    queries = [
        # (a description is walked must, must_not, filter, should)
        # leaves: 0 {t0, t1|-}, 1 {t2|-}, 2 {t2|t1}, 3 {t1}, 4 filter 1, 5 filter 0
        # nodes: 0 bool{must_not l1, filter l4} under must, 1 dis_max(l2), 2 the root
        {"bool": {"should": [{"dis_max": [T((2, 1))]}, T(1)],
                  "must": [T((0, 0), (1, N.NO_TERM)), {"bool": {"must_not": [T((2, N.NO_TERM))], "filter": [1]}}],
                  "filter": [0], "minimum_should_match": 1}},
        None,
        # leaves: 0 {t1} under the dis_max, 1 {t2|-} straight under the root's must, 2 filter 1
        {"bool": {"must": [{"dis_max": [T((1, 1))]}, T((2, N.NO_TERM))], "filter": [1]}},
    ]
    rc, msg, t = plan_tree(queries, offs)
    assert rc == N.OK, msg
    # term_begin, n_terms, node_begin, n_nodes, n_leaves, filt_begin, n_filters, pad
    assert t["queries"] == [[0, 5, 0, 3, 6, 0, 2, 0], [5, 0, 3, 0, 0, 2, 0, 0], [5, 2, 3, 2, 3, 2, 1, 0]]
    b = lambda *bits: sum(1 << x for x in bits)
    assert t["nodes"] == [
        (b(4), b(1), 0, 0),                # node 0: the nested bool — filter leaf 4 MUST, leaf 1 MUST_NOT
        (0, 0, b(2), 1),                   # node 1: the dis_max over leaf 2
        (b(0, 32, 5), 0, b(33, 3), 1),     # the root: leaf 0, node 0, filter leaf 5 MUST; node 1, leaf 3 SHOULD
        (0, 0, b(0), 1),                   # query 2: the dis_max over leaf 0
        (b(32, 1, 2), 0, 0, 0),            # its root: the dis_max, leaf 1 and the filter leaf MUST
    ]
    # rows: leaves 0 and 1 reach the root over MUST / MUST_NOT edges only and come first; then leaves 2 and 3
    assert t["terms"][0:5] == [(0, 3, 0), (3 + 64, 0, 0 | END), (3 + 128, 7, 1 | END), (3 + 128, 7, 2 | END), (3 + 64, 0, 3 | END)]
    assert t["terms"][5:10] == [(0, 5, 0), (0, 0, 0 | END), (0, 0, 1 | END), (5 + 64, 4, 2 | END), (5 + 64, 4, 3 | END)]
    # query 2: leaf 1 reaches the root over a MUST edge and goes first; leaf 0 hangs under a SHOULD edge
    assert t["terms"][10:12] == [(3 + 128, 7, 1 | END), (3 + 64, 0, 0 | END)]
    assert t["terms"][12:] == [(0, 0, 1 | END), (5 + 64, 4, 0 | END)]
    assert t["filt_rows"] == [0, 1, 0]  # query 0: filters 1 then 0; query 2: filter 1 again, the same row
    addr = lambda f, s: ((f + 1) << 32) | (s << 8) | 3
    assert t["filters"] == [addr(1, 0), addr(1, 1), addr(0, 0), addr(0, 1)]


def test_planned_node_masks_equal_the_models():
    rng = np.random.default_rng(77)
    offs = [np.arange(13) * 3]
    for _ in range(30):
        d = R.random_tree(rng, 12, 4, {"leaves": 32, "nodes": 32}, filter_ids=(0, 1))
        rc, msg, t = plan_tree([d], offs)
        assert rc == 0, msg
        assert t["nodes"] == R.compiled_nodes(BT.compile_matchers([d], 1), 0)
    rc, msg, t = plan_tree([chain(32)], offs)
    assert rc == 0 and len(t["nodes"]) == 32 and t["nodes"] == R.compiled_nodes(BT.compile_matchers([chain(32)], 1), 0)
    # (leaves are numbered as the description is walked, from the root down: the root holds leaf 0, node 0 leaf 31)
    assert t["nodes"][31][0] | t["nodes"][31][1] | t["nodes"][31][2] == (1 << 0) | (1 << 62)
    assert t["nodes"][0] == (1 << 31, 0, 0, 0)


# ---- the three-valued rule ----
def node_words(nodes):
    w = np.zeros((max(len(nodes), 1), 8), np.uint32)
    for i, (must, must_not, should, ms) in enumerate(nodes):
        w[i] = [must & 0xFFFFFFFF, must >> 32, must_not & 0xFFFFFFFF, must_not >> 32, should & 0xFFFFFFFF, should >> 32, ms, 0]
    return w


class Rule:
    """slg::booltree_eval over one compiled tree"""

    def __init__(self, d):
        tree = BT.compile_matchers([d], 1)
        self.nodes = R.compiled_nodes(tree, 0)
        self.n_leaves = int(tree["g_offsets"][1]) + int(tree["f_offsets"][1])
        self.words = node_words(self.nodes)
        self.root = 1 << (31 + len(self.nodes))
        self.L = plan_lib()

    def eval(self, t, f):
        """-> (t, f) with the decided nodes' bits"""
        tt, ff = C.c_uint64(t), C.c_uint64(f)
        self.L.slgp_booltree_eval(C.c_void_p(self.words.ctypes.data), len(self.nodes), C.byref(tt), C.byref(ff))
        assert tt.value & ff.value == 0 and tt.value & 0xFFFFFFFF == t and ff.value & 0xFFFFFFFF == f
        return tt.value, ff.value

    def root3(self, t, f):
        """the root under what is known: True, False or None (open)"""
        tt, ff = self.eval(t, f)
        return True if tt & self.root else (False if ff & self.root else None)

    def value(self, t):
        """the root's value with every leaf known, by the model's two-valued evaluation (independent of the rule)"""
        v = t
        for i, (must, must_not, should, ms) in enumerate(self.nodes):
            if v & must == must and v & must_not == 0 and bin(v & should).count("1") >= ms:
                v |= 1 << (32 + i)
        return bool(v & self.root)


def check_exhaustively(d):
    """every partial assignment of the tree's leaves (3 ^ n): a decided root equals the root of every completion,
    and with all leaves known the root is decided and equals the two-valued value"""
    r = Rule(d)
    n = r.n_leaves
    assert n <= 6
    full = [r.value(t) for t in range(1 << n)]
    decided = 0
    for state in itertools.product((0, 1, 2), repeat=n):  # per leaf: false, true, open
        t = sum(1 << i for i, s in enumerate(state) if s == 1)
        f = sum(1 << i for i, s in enumerate(state) if s == 0)
        open_bits = [i for i, s in enumerate(state) if s == 2]
        got = r.root3(t, f)
        outcomes = {full[t | sum(1 << i for i, on in zip(open_bits, fill) if on)]
                    for fill in itertools.product((0, 1), repeat=len(open_bits))}
        if got is not None:
            assert outcomes == {got}, (d, state, got, outcomes)
            decided += 1
        if not open_bits:
            assert got is not None and got == full[t], (d, state)
    return decided


KINDS = [
    T(0), "match_all", {"dis_max": []}, {"dis_max": [T(0), T(1), T(2)]}, {"query_string": {}},
    {"query_string": {"not": [[0], [1]]}}, {"query_string": {"terms": [[0], [1], [2]], "not": [[3]], "minimum_should_match": 2}},
    {"bool": {"must": [T(0), T(1)], "must_not": [T(2)], "should": [T(3), T(4)], "filter": [0]}},
    {"bool": {"should": [T(0), T(1), T(2)], "minimum_should_match": 2}},
    {"bool": {"should": [T(0), T(1)], "minimum_should_match": 3}},
    {"bool": {"must_not": [{"bool": {"must_not": [T(0)]}}], "should": [{"dis_max": []}, "match_all"]}},
]
DEPTH4 = {"bool": {"must": [{"bool": {"should": [{"bool": {"must_not": [{"dis_max": [T(0), T(1)]}], "must": [T(2)]}}, T(3)]}}],
                   "must_not": [{"query_string": {"terms": [[4]], "not": [[5]]}}]}}


@pytest.mark.parametrize("i", range(len(KINDS)))
def test_three_valued_rule_every_node_kind(i):
    check_exhaustively(KINDS[i])


def test_three_valued_rule_depth_4():
    assert check_exhaustively(DEPTH4) > 64  # (decided well before every leaf is known, too)


def test_three_valued_rule_exhaustive_small_trees():
    """40 random trees of at most 6 leaves (fixed seed), 3 ^ leaves partial assignments each"""
    rng = np.random.default_rng(4242)
    seen = 0
    while seen < 40:
        d = R.random_tree(rng, 12, 4, {"leaves": 6, "nodes": 8}, filter_ids=(0,))
        check_exhaustively(d)
        seen += 1


def test_three_valued_rule_32_node_chain():
    """the 32-node chain (32 leaves, the root is bit 63): the leaves cannot be enumerated, so 400 random partial
    assignments (fixed seed), each against 32 random completions and the all-false / all-true ones; and the
    assignments that decide the root by its own leaf alone, or leave it open down to node 0"""
    r = Rule(chain(32))
    assert len(r.nodes) == 32 and r.n_leaves == 32 and r.root == 1 << 63
    rng = np.random.default_rng(63)
    decided = 0
    for _ in range(400):
        p_open = rng.choice([0.0, 0.1, 0.5, 0.9])
        state = np.where(rng.random(32) < p_open, 2, rng.integers(0, 2, 32))
        t = sum(1 << i for i in range(32) if state[i] == 1)
        f = sum(1 << i for i in range(32) if state[i] == 0)
        open_mask = sum(1 << i for i in range(32) if state[i] == 2)
        got = r.root3(t, f)
        fills = [0, open_mask] + [int(rng.integers(0, 1 << 32)) & open_mask for _ in range(32)]
        outcomes = {r.value(t | x) for x in fills}
        if got is not None:
            assert outcomes == {got}
            decided += 1
        if open_mask == 0:
            assert got is not None
    assert decided >= 100
    own = [(m | mn | sh) & 0xFFFFFFFF for m, mn, sh, _ in r.nodes]  # each node's own leaf, as a bit
    assert own[31] == 1 << 0 and own[0] == 1 << 31
    # the root (node 31, odd: should [leaf, node 30], min_should 1) is decided by its own leaf alone ...
    assert r.root3(own[31], 0) is True
    # ... and with the leaves of the odd nodes false and those of the even nodes true every node is the one below it
    # (odd) or its negation (even): the root hangs on node 0's leaf, open until that last leaf is known
    t = sum(own[i] for i in range(2, 32, 2))
    f = sum(own[i] for i in range(1, 32, 2))
    assert r.root3(t, f) is None
    assert r.root3(t | own[0], f) == r.value(t | own[0]) and r.root3(t, f | own[0]) == r.value(t)
    assert r.value(t | own[0]) != r.value(t)
