"""slg_index_add_nested_filter_trees argument checks that need no device, through the host planner
(slgp_plan_nested_filter_trees: check_nested_filter_trees + plan_nested_filter_trees, pure host code): every error
of the header's list, in its order (SLG_ERR_INVALID for what needs no index; the limits; ids, kinds and ordinals
against the state; the doc level's 2^53 rule), the image of a known tree, and the struct layouts of the header against
the ctypes binding and the Rust mirror."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_filter_args import Field, NODE_DT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW, F64, I64, FID, AND, OR, NOT, NESTED = range(8)
EXPORTS = {"slg_index_add_nested_path": 5, "slg_index_remove_nested_path": 2, "slg_index_add_nested_field_f64": 5,
           "slg_index_add_nested_field_i64": 5, "slg_index_add_nested_field_ord": 6, "slg_index_remove_nested_field": 2,
           "slg_index_add_nested_filter_trees": 4}

kw = lambda field=0, begin=0, n=0: dict(kind=KW, field=field, ord_begin=begin, n_ords_in=n)
f64 = lambda field=1, lo=0.0, hi=1.0: dict(kind=F64, field=field, lo_f=lo, hi_f=hi)
i64 = lambda field=2, lo=0, hi=1: dict(kind=I64, field=field, lo_i=lo, hi_i=hi)
fid = lambda f=0: dict(kind=FID, filter_id=f)
AND_ = lambda n: dict(kind=AND, arity=n)
OR_ = lambda n: dict(kind=OR, arity=n)
NOT_ = dict(kind=NOT)
nested = lambda scope: dict(kind=NESTED, field=scope)


class Path(C.Structure):
    _fields_ = [("id", C.c_int32), ("parent", C.c_int32), ("seg_has", C.c_void_p)]


class NField(C.Structure):
    _fields_ = [("id", C.c_int32), ("path", C.c_int32), ("kind", C.c_uint32), ("n_ords", C.c_uint32), ("seg_has", C.c_void_p)]


# the state: agg fields 0 keyword(33), 1 f64, 2 i64 within 2^53, 5 i64 beyond it; paths 0 <- 1 <- 2 <- 3 <- 4, 7 without
# tables for segment 1; nested fields 0 keyword(33) / 1 f64 / 2 i64 under path 0, 3 keyword(5) under path 1, 4 f64
# under path 0 without a column for segment 1
FIELDS = {0: dict(keyword=1, n_ords=33), 1: {}, 2: dict(from_i64=1, vmin=-5.0, vmax=2.0 ** 53),
          5: dict(from_i64=1, vmin=0.0, vmax=2.0 ** 53 + 2.0)}
PATHS = {0: dict(parent=-1), 1: dict(parent=0), 2: dict(parent=1), 3: dict(parent=2), 4: dict(parent=3),
         7: dict(parent=-1, has=[1, 0])}
NFIELDS = {0: dict(path=0, kind=3, n_ords=33), 1: dict(path=0, kind=1), 2: dict(path=0, kind=2),
           3: dict(path=1, kind=3, n_ords=5), 4: dict(path=0, kind=1, has=[1, 0])}
SCOPE_DT = np.dtype([("node_begin", "<u4"), ("n_nodes", "<u4"), ("path_row", "<u4"), ("pad", "<u4")])


def tree(*scopes, ords=()):
    """scopes: (path, [nodes]) in order -> a (scopes, nodes, ords) triple"""
    rows, nodes = [], []
    for path, prog in scopes:
        rows.append((path, len(nodes), len(prog)))
        nodes += prog
    return rows, nodes, list(ords)


LEAF = tree((-1, [f64()]))
ONE = tree((0, [f64(1)]), (-1, [nested(0)]))


def plan(trees, filter_live=(), n_segs=2, arr=None, n_trees=None):
    """-> (code, message, scope rows, node records, level_begin, bit-set words, [path rows, nested column rows])"""
    from searchlite_amd import build
    from searchlite_amd.filters import nested_tree_array
    L = C.CDLL(build.build_plan_lib())
    L.slgp_plan_nested_filter_trees.restype = C.c_int
    keep = []

    def has(d):
        a = np.array(d.get("has", [1] * n_segs), np.uint8)
        keep.append(a)
        return a.ctypes.data

    fa = (Field * len(FIELDS))()
    for i, (id_, f) in enumerate(FIELDS.items()):
        dense = np.zeros(n_segs, np.uint8)
        keep.append(dense)
        fa[i] = Field(id_, int(f.get("keyword", 0)), int(f.get("n_ords", 0)), int(f.get("from_i64", 0)), 1,
                      f.get("vmin", 0.0), f.get("vmax", 0.0), has(f), dense.ctypes.data)
    pa = (Path * len(PATHS))(*[Path(i, p["parent"], has(p)) for i, p in PATHS.items()])
    na = (NField * len(NFIELDS))(*[NField(i, f["path"], f["kind"], f.get("n_ords", 0), has(f)) for i, f in NFIELDS.items()])
    live = np.array(list(filter_live) + [0], np.uint8)
    ta, keep2 = nested_tree_array(trees)
    scopes, nodes = np.zeros(2048, SCOPE_DT), np.zeros(8192, NODE_DT)
    levels, words = np.zeros(16, np.uint32), np.zeros(1024, np.uint32)
    counts, err = (C.c_uint32 * 6)(), C.create_string_buffer(256)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = L.slgp_plan_nested_filter_trees(fa, len(FIELDS), p(live), len(filter_live), pa, len(PATHS), na, len(NFIELDS), n_segs,
                                         ta if arr is None else arr, len(trees) if n_trees is None else n_trees,
                                         p(scopes), 2048, p(nodes), 8192, p(levels), 16, p(words), 1024, counts, err, 256)
    return (rc, err.value.decode(), scopes[:counts[0]], nodes[:counts[1]], levels[:counts[2]].tolist(),
            words[:counts[3]].tolist(), [counts[4], counts[5]])


def rejected(trees, code, word, **kw_):
    from searchlite_amd import _native as N
    rc, msg = plan(trees, **kw_)[:2]
    assert rc == getattr(N, code) and word in msg, (rc, msg)


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


@pytest.mark.parametrize("name", sorted(EXPORTS))
def test_export_and_argument_counts(lib, name):
    assert hasattr(lib, name), f"{name} is not exported"
    assert len(getattr(lib, name).argtypes) == EXPORTS[name]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "searchlite_gpu.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, header, re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == EXPORTS[name]
    rs = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    m = re.search(r"pub fn %s\((.*?)\)\s*->" % name, rs, re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == EXPORTS[name]


def test_struct_layouts_and_constants_match_the_header_and_the_rust_mirror(tmp_path):
    from searchlite_amd import _native as N
    consts = {"SLG_FILTER_NESTED": 7, "SLG_MAX_NESTED_SCOPES": 16, "SLG_MAX_NESTED_DEPTH": 4}
    structs = {"slg_nested_scope": N.NestedScope, "slg_nested_filter_tree": N.NestedFilterTree, "slg_filter_node": N.FilterNode}
    body = ""
    for name, cls in structs.items():
        body += '  printf(" %%zu", sizeof(%s));\n' % name
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f, _ in cls._fields_)
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n' + body +
                   "".join('  printf(" %%d", (int)%s);\n' % c for c in consts) + "  return 0;\n}\n")
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    ffi = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    for name, cls in structs.items():
        fields = [f for f, _ in cls._fields_]
        assert out[0] == C.sizeof(cls), name
        assert out[1:1 + len(fields)] == [getattr(cls, f).offset for f in fields], name
        out = out[1 + len(fields):]
        rust = re.search(r"pub struct %s \{(.*?)\}" % name, ffi, re.S).group(1)
        assert re.findall(r"pub\s+(\w+)\s*:", rust) == fields
    assert out == list(consts.values())
    for name, val in consts.items():
        assert getattr(N, name[4:]) == val
        assert re.search(r"pub const %s: \w+ = %d;" % (name, val), ffi), name
    assert SCOPE_DT.itemsize == 16 and NODE_DT.itemsize == 32


def test_a_null_index_fails_behind_the_checks_of_the_trees(lib):
    from searchlite_amd import _native as N
    from searchlite_amd.filters import nested_tree_array
    ids = np.full(1, -7, np.int32)
    for trees, word in (([ONE], "index is NULL"), ([tree((0, [fid()]), (-1, [nested(0)]))], "FILTER_ID in an object scope")):
        a, keep = nested_tree_array(trees)
        assert lib.slg_index_add_nested_filter_trees(None, a, 1, ids.ctypes.data) == N.ERR_INVALID
        assert word.encode() in lib.slg_last_error() and ids[0] == -7
    a, keep = nested_tree_array([ONE])
    assert lib.slg_index_add_nested_filter_trees(None, a, 1, None) == N.ERR_INVALID
    assert b"out_ids is NULL" in lib.slg_last_error()
    for call in (lambda: lib.slg_index_add_nested_path(None, -1, None, None, None),
                 lambda: lib.slg_index_remove_nested_path(None, 0),
                 lambda: lib.slg_index_add_nested_field_f64(None, 0, None, None, None),
                 lambda: lib.slg_index_add_nested_field_i64(None, 0, None, None, None),
                 lambda: lib.slg_index_add_nested_field_ord(None, 0, None, None, None, 1),
                 lambda: lib.slg_index_remove_nested_field(None, 0)):
        assert call() == N.ERR_INVALID and b"index is NULL" in lib.slg_last_error()


def test_null_and_empty_arguments():
    from searchlite_amd import _native as N
    assert plan([LEAF])[0] == N.OK and plan([ONE])[0] == N.OK
    rejected([], "ERR_INVALID", "trees is NULL", arr=C.c_void_p(None), n_trees=1)
    rejected([], "ERR_INVALID", "n_trees is 0")
    rejected([([], [f64()], [])], "ERR_INVALID", "n_scopes is 0")
    nodes = (N.FilterNode * 1)(N.FilterNode(kind=KW, n_ords_in=0))
    scopes = (N.NestedScope * 1)(N.NestedScope(-1, 0, 1))
    rejected([LEAF], "ERR_INVALID", "scopes is NULL", arr=(N.NestedFilterTree * 1)(N.NestedFilterTree(1, None, 1, C.addressof(nodes), 0, None)))
    rejected([LEAF], "ERR_INVALID", "n_nodes is 0", arr=(N.NestedFilterTree * 1)(N.NestedFilterTree(1, C.addressof(scopes), 0, C.addressof(nodes), 0, None)))
    rejected([LEAF], "ERR_INVALID", "nodes is NULL", arr=(N.NestedFilterTree * 1)(N.NestedFilterTree(1, C.addressof(scopes), 1, None, 0, None)))
    rejected([LEAF], "ERR_INVALID", "ords is NULL", arr=(N.NestedFilterTree * 1)(N.NestedFilterTree(1, C.addressof(scopes), 1, C.addressof(nodes), 2, None)))


@pytest.mark.parametrize("bad,word", [
    (tree((0, [f64(1)])), "the last scope is not the doc level"),
    (tree((-1, [f64()]), (-1, [f64()])), "a scope before the last one is the doc level"),
    (tree((-2, [f64()]), (-1, [nested(0)])), "path below -1"),
    (([(0, 0, 0), (-1, 0, 1)], [nested(0)], []), "the scope's n_nodes is 0"),
    (([(0, 0, 1), (-1, 1, 1)], [f64(1)], []), "node_begin + n_nodes > the tree's n_nodes"),
    (([(0, 0xFFFFFFFF, 2), (-1, 0, 1)], [nested(0)], []), "node_begin + n_nodes > the tree's n_nodes"),
    (tree((0, [dict(kind=8)]), (-1, [nested(0)])), "unknown filter node kind"),
    (tree((0, [dict(kind=-1)]), (-1, [nested(0)])), "unknown filter node kind"),
    (tree((0, [NOT_]), (-1, [nested(0)])), "NOT underflows the stack"),
    (tree((0, [f64(1), AND_(2)]), (-1, [nested(0)])), "arity larger than the stack"),
    (tree((0, [f64(1), f64(1)]), (-1, [nested(0)])), "does not end with exactly one value"),
    (tree((0, [f64(1)]), (-1, [nested(0), f64()])), "does not end with exactly one value"),
    (tree((0, [f64(1, lo=float("nan"))]), (-1, [nested(0)])), "NaN bound"),
    (tree((0, [kw(0, 1, 2)]), (-1, [nested(0)]), ords=[0, 1]), "ord_begin + n_ords_in > n_ords"),
    (tree((0, [fid(0)]), (-1, [nested(0)])), "FILTER_ID in an object scope"),
    (tree((0, [nested(0)]), (-1, [nested(0)])), "a NESTED node names no earlier scope"),
    (tree((0, [f64(1)]), (-1, [nested(1)])), "a NESTED node names no earlier scope"),
    (tree((0, [f64(1)]), (-1, [nested(-1)])), "a NESTED node names no earlier scope"),
    (tree((0, [f64(1)]), (-1, [nested(0), nested(0), AND_(2)])), "named by more than one NESTED node"),
    (tree((0, [f64(1)]), (0, [f64(1)]), (-1, [nested(1)])), "named by no NESTED node"),
])
def test_invalid_trees(bad, word):
    rejected([LEAF, bad], "ERR_INVALID", word)
    rejected([LEAF, bad], "ERR_INVALID", "in nested filter tree 1")


def chain(depth, leaf=None):
    """object scopes of paths depth - 1, ..., 0 below one another"""
    scopes = [(depth - 1, [leaf or OR_(0)])] + [(depth - 2 - i, [nested(i)]) for i in range(depth - 1)]
    return tree(*scopes, (-1, [nested(depth - 1)]))


def test_the_limits_are_unsupported_and_come_behind_every_invalid_argument():
    from searchlite_amd import _native as N
    wide15 = tree(*[(0, [f64(1)])] * 15, (-1, [nested(i) for i in range(15)] + [OR_(15)]))     # 16 scopes, 31 nodes
    wide16 = tree(*[(0, [f64(1)])] * 16, (-1, [nested(i) for i in range(16)] + [OR_(16)]))     # 17 scopes
    nodes64 = tree((0, [f64(1)] + [NOT_] * 61), (-1, [nested(0), NOT_]))                         # 64 nodes over both
    nodes65 = tree((0, [f64(1)] + [NOT_] * 62), (-1, [nested(0), NOT_]))
    deep16 = tree((0, [f64(1)] * 16 + [AND_(16)]), (-1, [nested(0)]))
    deep17 = tree((0, [f64(1)] * 17 + [AND_(17)]), (-1, [nested(0)]))
    for ok in (wide15, nodes64, deep16, chain(4)):
        rc, msg = plan([ok])[:2]
        assert rc == N.OK, msg
    assert plan([LEAF] * 64)[0] == N.OK
    rejected([nodes65], "ERR_UNSUPPORTED", "SLG_MAX_FILTER_NODES")
    rejected([deep17], "ERR_UNSUPPORTED", "SLG_MAX_FILTER_DEPTH")
    rejected([wide16], "ERR_UNSUPPORTED", "SLG_MAX_NESTED_SCOPES")
    rejected([chain(5)], "ERR_UNSUPPORTED", "SLG_MAX_NESTED_DEPTH")
    rejected([LEAF] * 65, "ERR_UNSUPPORTED", "SLG_MAX_FILTER_TREES")
    # an invalid argument anywhere comes first, also in a later tree and in the 65th of a call
    rejected([chain(5), tree((0, [NOT_]), (-1, [nested(0)]))], "ERR_INVALID", "underflows")
    rejected([LEAF] * 64 + [tree((-1, [dict(kind=9)]))], "ERR_INVALID", "unknown filter node kind")
    # and the limits come before anything is looked up in the state
    rejected([chain(5, leaf=f64(99))], "ERR_UNSUPPORTED", "SLG_MAX_NESTED_DEPTH")
    rejected([tree((99, [f64(1)]), (-1, [nested(0)]))] * 65, "ERR_UNSUPPORTED", "SLG_MAX_FILTER_TREES")


def test_ids_kinds_and_ordinals_against_the_state():
    from searchlite_amd import _native as N
    one = lambda path, node, ords=(): tree((path, [node]), (-1, [nested(0)]), ords=ords)
    for bad, word in ((one(9, f64(1)), "unknown nested path id 9"),
                      (one(7, OR_(0)), "nested path 7 has no tables for segment 1"),
                      (one(0, f64(9)), "unknown nested field id 9"),
                      (one(0, f64(4)), "nested field 4 has no column for segment 1"),
                      (one(0, kw(1)), "nested field 1 is not a keyword field"),
                      (one(0, f64(0)), "nested field 0 is not an f64 field"),
                      (one(0, f64(2)), "nested field 2 is not an f64 field"),
                      (one(0, i64(1)), "nested field 1 is not an i64 field"),
                      (one(0, kw(0, 0, 2), [32, 33]), "ordinal 33 >= n_ords of nested field 0"),
                      (tree((2, [OR_(0)]), (0, [nested(0)]), (-1, [nested(1)])), "nested path 2 is not registered under path 0"),
                      (tree((0, [OR_(0)]), (1, [nested(0)]), (-1, [nested(1)])), "nested path 0 is not registered under path 1"),
                      (tree((0, [f64(1)]), (-1, [nested(0), kw(9), AND_(2)])), "unknown agg field id 9"),
                      (tree((0, [f64(1)]), (-1, [nested(0), fid(3), AND_(2)])), "unknown filter id 3"),
                      (tree((0, [f64(1)]), (-1, [nested(0), f64(0), AND_(2)])), "is a keyword field")):
        rc, msg = plan([LEAF, bad], filter_live=[1, 0])[:2]
        assert rc == N.ERR_INVALID and word in msg and "in nested filter tree 1" in msg, (bad, rc, msg)
    # a path with a parent is fine at the doc level: no parent test is made there
    assert plan([tree((2, [OR_(0)]), (-1, [nested(0)]))])[0] == N.OK
    # the doc level keeps the 2^53 rule, behind every invalid argument; nested i64 columns know no such rule
    big = tree((0, [i64(2, -2**63, 2**63 - 1)]), (-1, [nested(0), i64(5), AND_(2)]))
    rejected([big], "ERR_UNSUPPORTED", "2^53")
    rejected([big, one(0, f64(9))], "ERR_INVALID", "unknown nested field id 9")


def test_the_planned_image_of_known_trees():
    """rows by level, the doc-level scopes last in tree order; NESTED rows name scope rows; int64 bounds travel as
    bits; a column of another path is OR of nothing"""
    from searchlite_amd import _native as N
    t0 = tree((1, [kw(3, 0, 2)]), (0, [kw(0, 2, 1), nested(0), i64(2, -2**63, 2**53 + 1), AND_(3)]),
              (-1, [nested(1), NOT_]), ords=[4, 0, 32])
    t1 = tree((0, [f64(1, -0.5, float("inf"))]), (0, [kw(3, 0, 1)]), (-1, [nested(0), nested(1), i64(2, -7, 2**60), OR_(3)]), ords=[1])
    t2 = tree((-1, [f64(1)]))
    rc, msg, scopes, nodes, levels, words, tables = plan([t0, t1, t2])
    assert rc == N.OK, msg
    # level 1: t0's scope 0, t1's scopes 0 and 1; level 2: t0's scope 1; then the doc levels of t0, t1, t2
    assert levels == [0, 3, 4] and len(scopes) == 7
    assert scopes["n_nodes"].tolist() == [1, 1, 1, 4, 2, 4, 1]
    assert scopes["node_begin"].tolist() == [0, 1, 2, 3, 7, 9, 13]
    assert scopes["path_row"].tolist()[:4] == [0, 1, 1, 1] and tables == [2, 4]   # paths 1, 0; nested fields 3, 0, 2, 1
    assert nodes["kind"].tolist() == [KW, F64, OR, KW, NESTED, I64, AND, NESTED, NOT, NESTED, NESTED, I64, OR, F64]
    assert nodes["row"][[4, 7, 9, 10]].tolist() == [0, 3, 1, 2]                  # NESTED: the child's scope row
    assert nodes["arity"][2] == 0                                                # t1's scope 1: a path-1 column under path 0
    assert nodes["row"][[0, 3, 5, 1]].tolist() == [0, 1, 2, 3]
    assert nodes["bits"][[0, 3]].tolist() == [0, 1] and words[:3] == [1 << 4 | 1, 0, 1]   # {4, 0} of 5 keys; {32} of 33
    as_i64 = lambda x: int(np.array([x], "<f8").view("<i8")[0])
    assert (as_i64(nodes["lo"][5]), as_i64(nodes["hi"][5])) == (-2**63, 2**53 + 1)   # nested: int64 bits, not clamped
    assert (nodes["lo"][11], nodes["hi"][11]) == (-7.0, 2.0 ** 53)                   # doc level: clamped into 2^53


# ---- check and plan under the sanitizers ---------------------------------------------------------------------
def test_check_and_plan_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/nested_filter_sanitize.cpp, a stand-alone program: pseudo-random trees, half of them with wild kinds,
    ids, arities and node ranges, through check_nested_filter_trees and plan_nested_filter_trees, built with
    -fsanitize=address,undefined"""
    csrc = os.path.join(ROOT, "searchlite_amd", "csrc")
    exe = str(tmp_path / "nested_filter_sanitize")
    # (the sanitizers' runtimes linked into the program itself: it needs nothing from the environment it runs in)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "nested_filter_sanitize.cpp"),
                           os.path.join(csrc, "slg_plan.cpp")])
    out = subprocess.run([exe, "4000", "2026"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    counts = {k: int(v) for k, v in (kv.split("=") for kv in out.stdout.split())}
    assert counts["trees"] >= 4000 and counts["ok"] + counts["invalid"] + counts["unsupported"] == 4000
    assert counts["ok"] > 400 and counts["invalid"] > 400 and counts["unsupported"] > 40, counts
