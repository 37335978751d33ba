"""slg_index_add_filter_trees / slg_index_fetch_filter argument checks that need no device: the trees are checked
before the index is looked at (a NULL index then fails with SLG_ERR_INVALID and a message, before anything touches a
GPU); field ids, filter ids, column kinds, ordinals, the 2^53 rule and the image the kernel reads are checked through
the host planner (plan_filter_trees: pure host code); the header, the ctypes binding and the Rust mirror agree on
the argument counts, the structs and the constants."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {"slg_index_add_filter_trees": 4, "slg_index_fetch_filter": 4}
KW, F64, I64, FID, AND, OR, NOT = range(7)

kw = lambda field=0, begin=0, n=0: dict(kind=KW, field=field, ord_begin=begin, n_ords_in=n)
f64 = lambda field=1, lo=0.0, hi=1.0: dict(kind=F64, field=field, lo_f=lo, hi_f=hi)
i64 = lambda field=2, lo=0, hi=1: dict(kind=I64, field=field, lo_i=lo, hi_i=hi)
fid = lambda f=0: dict(kind=FID, filter_id=f)
AND_ = lambda n: dict(kind=AND, arity=n)
OR_ = lambda n: dict(kind=OR, arity=n)
NOT_ = dict(kind=NOT)
LEAF = ([f64()], [])


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


def add(lib, trees, n_trees=None, null_ids=False, arr=None):
    """slg_index_add_filter_trees on a NULL index -> (code, message); no id may be written"""
    from searchlite_amd.filters import tree_array
    a, keep = tree_array(trees)
    ids = np.full(max(len(trees), 1), -7, np.int32)
    rc = lib.slg_index_add_filter_trees(None, a if arr is None else arr, len(trees) if n_trees is None else n_trees,
                                        None if null_ids else ids.ctypes.data)
    assert (ids == -7).all()
    assert lib.slg_last_error_code() == rc
    return rc, lib.slg_last_error().decode()


def rejected(lib, trees, code, word, **kw_):
    from searchlite_amd import _native as N
    rc, msg = add(lib, trees, **kw_)
    assert rc == getattr(N, code) and word in msg, (rc, msg)


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


def test_struct_layouts_and_constants_match_the_header_and_the_rust_mirror(tmp_path, lib):
    import subprocess
    from searchlite_amd import _native as N
    consts = ["SLG_FILTER_KEYWORD_IN", "SLG_FILTER_RANGE_F64", "SLG_FILTER_RANGE_I64", "SLG_FILTER_ID", "SLG_FILTER_AND",
              "SLG_FILTER_OR", "SLG_FILTER_NOT", "SLG_MAX_FILTER_NODES", "SLG_MAX_FILTER_DEPTH", "SLG_MAX_FILTER_TREES"]
    structs = {"slg_filter_node": N.FilterNode, "slg_filter_tree": N.FilterTree}
    src = tmp_path / "size.c"
    body = ""
    for name, cls in structs.items():
        body += '  printf(" %%zu", sizeof(%s));\n' % name
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f, _ in cls._fields_)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n' + body +
                   "".join('  printf(" %%d", (int)%s);\n' % c for c in consts) + '  return 0;\n}\n')
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
    values = dict(zip(consts, out))
    assert [values[c] for c in consts] == [0, 1, 2, 3, 4, 5, 6, 64, 16, 64]
    for name, val in values.items():
        assert getattr(N, name[4:]) == val, name
        assert re.search(r"pub const %s: \w+ = %d;" % (name, val), ffi), name
    assert lib.slg_abi_version() == 3


def test_valid_trees_reach_the_index(lib):
    """a valid call fails on the NULL index, after every check of the trees"""
    deep = [f64()] * 16 + [AND_(16)]                       # the stack reaches exactly SLG_MAX_FILTER_DEPTH
    wide = [f64()] + [NOT_] * 63                           # exactly SLG_MAX_FILTER_NODES nodes
    assert len(wide) == 64
    for trees in ([LEAF], [([AND_(0)], [])], [([OR_(0)], [])], [([f64(), NOT_, NOT_], [])], [(deep, [])],
                  [(wide, [])], [([kw(n=3)], [0, 1, 1])], [LEAF] * 64,
                  [([f64(lo=float("-inf"), hi=float("inf"))], [])], [([i64(lo=-2**63, hi=2**63 - 1)], [])]):
        rejected(lib, trees, "ERR_INVALID", "index is NULL")
    rejected(lib, [LEAF], "ERR_INVALID", "out_ids is NULL", null_ids=True)


def test_null_and_empty_arguments(lib):
    from searchlite_amd import _native as N
    rejected(lib, [], "ERR_INVALID", "trees is NULL", arr=C.c_void_p(None), n_trees=1)
    rejected(lib, [], "ERR_INVALID", "n_trees is 0")
    rejected(lib, [([], [])], "ERR_INVALID", "n_nodes is 0")
    one = (N.FilterTree * 1)(N.FilterTree(1, None, 0, None))
    rejected(lib, [LEAF], "ERR_INVALID", "nodes is NULL", arr=one)
    nodes = (N.FilterNode * 1)(N.FilterNode(kind=KW, n_ords_in=0))
    one = (N.FilterTree * 1)(N.FilterTree(1, C.addressof(nodes), 2, None))
    rejected(lib, [LEAF], "ERR_INVALID", "ords is NULL", arr=one)
    assert lib.slg_index_fetch_filter(None, 0, 0, None) == N.ERR_INVALID
    assert b"index is NULL" in lib.slg_last_error()


@pytest.mark.parametrize("nodes,ords,word", [
    ([dict(kind=7)], [], "unknown filter node kind"),
    ([dict(kind=-1)], [], "unknown filter node kind"),
    ([NOT_], [], "NOT underflows the stack"),
    ([f64(), AND_(2)], [], "arity larger than the stack"),
    ([OR_(1)], [], "arity larger than the stack"),
    ([f64(), f64()], [], "does not end with exactly one value"),
    ([f64(), f64(), f64(), AND_(2)], [], "does not end with exactly one value"),
    ([f64(lo=float("nan"))], [], "NaN bound"),
    ([f64(hi=float("nan"))], [], "NaN bound"),
    ([kw(begin=1, n=2)], [0, 1], "ord_begin + n_ords_in > n_ords"),
    ([kw(begin=0xFFFFFFFF, n=2)], [0, 1], "ord_begin + n_ords_in > n_ords"),
])
def test_invalid_programs(lib, nodes, ords, word):
    rejected(lib, [LEAF, (nodes, ords)], "ERR_INVALID", word)
    rejected(lib, [LEAF, (nodes, ords)], "ERR_INVALID", "in filter tree 1")


def test_limits_are_unsupported_and_come_behind_every_invalid_argument(lib):
    many = [f64()] + [NOT_] * 64                           # 65 nodes
    deep = [f64()] * 17 + [AND_(17)]
    rejected(lib, [(many, [])], "ERR_UNSUPPORTED", "SLG_MAX_FILTER_NODES")
    rejected(lib, [(deep, [])], "ERR_UNSUPPORTED", "SLG_MAX_FILTER_DEPTH")
    rejected(lib, [LEAF] * 65, "ERR_UNSUPPORTED", "SLG_MAX_FILTER_TREES")
    # an invalid argument anywhere is reported first: in a later tree, and in the 65th tree of a call
    rejected(lib, [(many, []), ([NOT_], [])], "ERR_INVALID", "underflows")
    rejected(lib, [(deep, []), ([f64(lo=float("nan"))], [])], "ERR_INVALID", "NaN bound")
    rejected(lib, [LEAF] * 64 + [([dict(kind=9)], [])], "ERR_INVALID", "unknown filter node kind")
    rejected(lib, [(many + [f64()], [])], "ERR_INVALID", "exactly one value")


# ---- against registered fields and filters: the host planner ------------------------------------------------
class Field(C.Structure):
    _fields_ = [("id", C.c_int32), ("keyword", C.c_uint32), ("n_ords", C.c_uint32), ("from_i64", C.c_uint32),
                ("any_value", C.c_uint32), ("vmin", C.c_double), ("vmax", C.c_double), ("seg_has", C.c_void_p),
                ("seg_dense", C.c_void_p)]


NODE_DT = np.dtype([("kind", "<u4"), ("arity", "<u4"), ("row", "<u4"), ("bits", "<u4"), ("lo", "<f8"), ("hi", "<f8")])
TWO53 = 2.0 ** 53
FIELDS = {0: dict(keyword=1, n_ords=33), 1: {}, 2: dict(from_i64=1, vmin=-5.0, vmax=TWO53),
          3: dict(keyword=1, n_ords=70, has=[1, 0]), 4: dict(from_i64=1, vmin=-TWO53 - 2.0, vmax=3.0),
          5: dict(from_i64=1, vmin=0.0, vmax=TWO53 + 2.0), 6: dict(from_i64=1, any_value=0), 7: dict(has=[0, 1])}


def plan(trees, fields=FIELDS, filter_live=(), n_segs=2):
    """-> (code, message, tree rows [n, 2], node records, column addresses [n, 2], filter addresses, bit-set words)
    of slgplan::check_filter_trees + plan_filter_trees"""
    from searchlite_amd import build
    from searchlite_amd.filters import tree_array
    L = C.CDLL(build.build_plan_lib())
    L.slgp_plan_filter_trees.restype = C.c_int
    keep, arr = [], (Field * max(len(fields), 1))()
    for i, (fid_, f) in enumerate(fields.items()):
        has = np.array(f.get("has", [1] * n_segs), np.uint8)
        dense = np.array(f.get("dense", [0] * n_segs), np.uint8)
        keep += [has, dense]
        arr[i] = Field(fid_, int(f.get("keyword", 0)), int(f.get("n_ords", 0)), int(f.get("from_i64", 0)),
                       int(f.get("any_value", 1)), f.get("vmin", 0.0), f.get("vmax", 0.0), has.ctypes.data, dense.ctypes.data)
    live = np.array(list(filter_live) + [0], np.uint8)
    ta, keep2 = tree_array(trees)
    rows, nodes = np.zeros((max(len(trees), 1), 2), np.uint32), np.zeros(256, NODE_DT)
    cols, flt, words = np.zeros((64, 2), np.uint64), np.zeros(64, np.uint64), np.zeros(256, np.uint32)
    counts, err = (C.c_uint32 * 4)(), C.create_string_buffer(256)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = L.slgp_plan_filter_trees(arr, len(fields), p(live), len(filter_live), n_segs, ta, len(trees), p(rows), p(nodes),
                                  256, p(cols), 64, p(flt), 64, p(words), 256, counts, err, 256)
    return rc, err.value.decode(), rows[:len(trees)], nodes[:counts[0]], cols[:counts[1]], flt[:counts[2]], words[:counts[3]]


def test_ids_kinds_and_ordinals_against_the_state():
    from searchlite_amd import _native as N
    assert NODE_DT.itemsize == 32
    ok = [([kw(0, 0, 2), f64(1), i64(2), fid(1), AND_(4)], [32, 0])]
    assert plan(ok, filter_live=[0, 1])[0] == N.OK
    for nodes, ords, word in (([kw(9)], [], "unknown agg field id 9"), ([f64(-1)], [], "unknown agg field id -1"),
                              ([fid(0)], [], "unknown filter id 0"), ([fid(2)], [], "unknown filter id 2"),
                              ([fid(-1)], [], "unknown filter id -1"),
                              ([kw(3)], [], "no column for segment 1"), ([f64(7)], [], "no column for segment 0"),
                              ([kw(1)], [], "not a keyword field"), ([f64(0)], [], "is a keyword field"),
                              ([i64(0)], [], "is a keyword field"), ([i64(1)], [], "not registered from i64"),
                              ([kw(0, 0, 2)], [32, 33], "ordinal 33 >= n_ords")):
        rc, msg = plan([LEAF, (nodes, ords)], filter_live=[0, 1])[:2]
        assert rc == N.ERR_INVALID and word in msg and "in filter tree 1" in msg, (nodes, rc, msg)
    # the checks that need no state come first, whatever the state would say
    rc, msg = plan([([kw(9)], []), ([NOT_], [])])[:2]
    assert rc == N.ERR_INVALID and "underflows" in msg
    rc, msg = plan([([kw(9)], [])] * 65)[:2]
    assert rc == N.ERR_UNSUPPORTED and "SLG_MAX_FILTER_TREES" in msg


def test_the_2_53_rule():
    """a column registered from i64 whose finite minimum or maximum lies beyond +-2^53 was rounded: RANGE_I64 over
    it is unsupported, behind every invalid argument; +-2^53 itself, and a column without a value, are fine; f64
    ranges over the same column are not refused"""
    from searchlite_amd import _native as N
    assert plan([([i64(2)], [])])[0] == N.OK and plan([([i64(6)], [])])[0] == N.OK
    for field in (4, 5):
        rc, msg = plan([([i64(field)], [])])[:2]
        assert rc == N.ERR_UNSUPPORTED and "2^53" in msg and f"agg field {field}" in msg, (rc, msg)
        assert plan([([f64(field)], [])])[0] == N.OK
        rc, msg = plan([([i64(field)], []), ([kw(9)], [])])[:2]
        assert rc == N.ERR_INVALID and "unknown agg field id 9" in msg


@pytest.mark.parametrize("lo,hi,want", [
    (-2**63, 2**63 - 1, (-TWO53, TWO53)), (2**63 - 1, -2**63, (float("inf"), float("-inf"))),
    (2**53, -2**53, (TWO53, -TWO53)), (2**53 + 1, 2**53 + 5, (float("inf"), TWO53)),
    (-2**53 - 5, -2**53 - 1, (-TWO53, float("-inf"))), (-7, 9, (-7.0, 9.0))])
def test_i64_bounds_are_clamped_into_2_53(lo, hi, want):
    rc, msg, _, nodes, *_ = plan([([i64(2, lo, hi)], [])])
    assert rc == 0, msg
    assert (nodes["lo"][0], nodes["hi"][0]) == want


def test_the_planned_image_of_a_known_tree():
    from searchlite_amd import _native as N
    fields = {0: dict(keyword=1, n_ords=33), 8: dict(keyword=1, n_ords=70, dense=[1, 0]), 2: dict(from_i64=1, vmin=-9.0, vmax=9.0),
              1: {}}
    t0 = ([kw(8, 1, 4), i64(2, -2**63, 2**63 - 1), f64(1, -0.0, float("inf")), AND_(3)], [5, 69, 32, 69, 0])
    t1 = ([fid(2), NOT_, kw(0, 0, 2), kw(0, 2, 0), i64(2, 2**53 + 1, -2**53 - 1), fid(0), OR_(4), OR_(2)], [32, 0])
    rc, msg, rows, nodes, cols, flt, words = plan([t0, t1], fields, filter_live=[1, 0, 1])
    assert rc == N.OK, msg
    assert rows.tolist() == [[0, 4], [4, 8]]
    assert nodes["kind"].tolist() == [KW, I64, F64, AND, FID, NOT, KW, KW, I64, FID, OR, OR]
    assert nodes["arity"].tolist() == [0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 4, 2]
    # rows of the two tables in order of first use: fields 8, 2, 1, 0; filters 2, 0
    assert nodes["row"].tolist() == [0, 1, 2, 0, 0, 0, 3, 3, 1, 1, 0, 0]
    # one bit set per KEYWORD_IN node: 3 words for n_ords 70, 2 words for n_ords 33 (twice)
    assert nodes["bits"][[0, 6, 7]].tolist() == [0, 3, 5] and len(words) == 7
    assert words.tolist() == [1 << 0, 1 << 0, 1 << 5, 1 << 0, 1 << 0, 0, 0]  # {69, 32, 69, 0}; {32, 0}; {}
    # INT64_MIN / INT64_MAX are clamped into +-2^53; a lower bound above 2^53 and an upper bound below -2^53 pass
    # nothing, also not a stored value of exactly +-2^53: the infinities; f64 bounds go through as they are
    assert (nodes["lo"][1], nodes["hi"][1]) == (-TWO53, TWO53)
    assert (nodes["lo"][8], nodes["hi"][8]) == (float("inf"), float("-inf"))
    assert nodes["hi"][2] == float("inf") and nodes["lo"][2] == 0.0 and np.signbit(nodes["lo"][2])
    addr = lambda owner, s, tag: ((owner + 1) << 32) | (s << 8) | tag
    assert cols.tolist() == [[0, addr(8, 0, 1)], [addr(8, 1, 2), addr(8, 1, 1)]] + \
        [[addr(f, s, 2), addr(f, s, 1)] for f in (2, 1, 0) for s in (0, 1)]
    assert flt.tolist() == [addr(2, 0, 3), addr(2, 1, 3), addr(0, 0, 3), addr(0, 1, 3)]
