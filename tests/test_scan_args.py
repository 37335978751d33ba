"""slg_batch_prepare_scan's checks and slice tables through the host planner (slgp_plan_scan: check_scan + plan_scan,
pure host code) before a device exists: every refusal with its code, the planned slices of segments around the
slice size with truncated and full regions, and the header, the ctypes binding and the Rust mirror agreeing on
argument counts, the spec's fields and the constants."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {"slg_batch_prepare_scan": 7, "slg_search_batch_scan": 15, "slg_batch_scan_info": 4}

MA = {"match_all": {}}
CS = lambda **kw: {"constant_score": kw}
RF = lambda field=0, **kw: {"rank_feature": dict(field=field, **kw)}


class Field(C.Structure):
    _fields_ = [("id", C.c_int32), ("keyword", C.c_uint32), ("non_finite", C.c_uint32), ("seg_has", C.c_void_p),
                ("seg_dense", C.c_void_p)]


@pytest.fixture(scope="module")
def plan_lib():
    from searchlite_amd import build
    L = C.CDLL(build.build_plan_lib())
    L.slgp_plan_scan.restype = C.c_int
    L.slgp_scan_slice_docs.restype = C.c_uint32
    return L


def spec_of(queries, **over):
    """scan.scan_spec; over: fields replaced by an array, or None for a NULL pointer -> (N.ScanSpec, keep)"""
    from searchlite_amd.scan import scan_spec
    sp, keep = scan_spec(queries)
    for name, v in over.items():
        if v is not None:
            keep[name] = np.ascontiguousarray(v, dtype=keep[name].dtype)
        setattr(sp, name, None if v is None else keep[name].ctypes.data)
    return sp, keep


def plan_scan(L, queries, seg_docs=(100, 50), fields=None, filter_live=(), q_filter=None, full_regions=False, k=11,
              spec=None, cap=4096):
    """-> dict(rc, msg, queries [nq, 8] words, qrefs [nq, 2], slices [n, 8], cbeg [n], cols [m, 2], root [nq], full,
    cand_total).  fields: {id: dict(keyword=, non_finite=, has=[per segment], dense=[per segment])}"""
    n_segs = len(seg_docs)
    fields = fields or {}
    keep, arr = [], (Field * max(len(fields), 1))()
    for i, (fid, f) in enumerate(fields.items()):
        has = np.array(f.get("has", [1] * n_segs), np.uint8)
        dense = np.array(f.get("dense", [0] * n_segs), np.uint8)
        keep += [has, dense]
        arr[i] = Field(fid, int(f.get("keyword", 0)), int(f.get("non_finite", 0)), has.ctypes.data, dense.ctypes.data)
    live = np.array(list(filter_live) + [0], np.uint8)
    sp, keep2 = (spec if spec is not None else spec_of(queries))
    nq = len(queries)
    docs = np.array(list(seg_docs) + [0], np.uint32)
    qf = None if q_filter is None else np.ascontiguousarray(q_filter, np.int32)
    qw, qr = np.zeros((max(nq, 1), 8), np.uint32), np.zeros((max(nq, 1), 2), np.uint32)
    sl, cbeg = np.zeros((cap, 8), np.uint32), np.zeros(cap, np.uint64)
    cols, root = np.zeros((64, 2), np.uint64), np.zeros(max(nq, 1), np.uint32)
    counts, err = (C.c_uint32 * 5)(), C.create_string_buffer(256)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    rc = L.slgp_plan_scan(p(docs), n_segs, arr, len(fields), p(live), len(filter_live), nq,
                          None if sp is None else C.byref(sp), p(qf), int(full_regions), k, p(qw), p(qr), p(sl), p(cbeg),
                          cap, p(cols), 64, p(root), counts, err, 256)
    return dict(rc=rc, msg=err.value.decode(), queries=qw[:nq], qrefs=qr[:nq], slices=sl[:counts[0]], cbeg=cbeg[:counts[0]],
                cols=cols[:counts[1]], root=root[:nq], full=counts[2], cand_total=counts[3] | (counts[4] << 32))


# ---- header, ctypes, Rust mirror ---------------------------------------------------------------------------
def _n_args(text, pattern):
    m = re.search(pattern, text, re.S)
    assert m, pattern
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(EXPORTS))
def test_export_and_argument_counts(name):
    from searchlite_amd import _native
    lib = _native.load()
    assert hasattr(lib, name), f"{name} is not exported"
    assert len(getattr(lib, name).argtypes) == EXPORTS[name]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "searchlite_gpu.h")).read(), flags=re.S)
    assert _n_args(header, r"\b%s\s*\((.*?)\)\s*;" % name) == EXPORTS[name]
    rs = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    assert _n_args(rs, r"pub fn %s\((.*?)\)\s*->" % name) == EXPORTS[name]


def test_spec_layout_matches_the_header_and_the_rust_mirror(tmp_path, plan_lib):
    import subprocess
    from searchlite_amd import _native as N
    consts = ["SLG_SCAN_MATCH_ALL", "SLG_SCAN_CONSTANT", "SLG_SCAN_RANK_FEATURE", "SLG_SCAN_MOD_NONE", "SLG_SCAN_MOD_LOG",
              "SLG_SCAN_MOD_LOG1P", "SLG_SCAN_MOD_SQRT", "SLG_SCAN_MOD_RECIPROCAL"]
    fields = [n for n, _ in N.ScanSpec._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(slg_scan_spec));\n' +
                   "".join('  printf(" %%zu", offsetof(slg_scan_spec, %s));\n' % f for f in fields) +
                   "".join('  printf(" %%d", (int)%s);\n' % c for c in consts) +
                   '  printf(" %u", (unsigned)SLG_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert out[0] == C.sizeof(N.ScanSpec)
    assert out[1:1 + len(fields)] == [getattr(N.ScanSpec, f).offset for f in fields]
    values = dict(zip(consts, out[1 + len(fields):]))
    ffi = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    for name, val in values.items():
        assert getattr(N, name[4:]) == val, name
        assert re.search(r"pub const %s: \w+ = %d;" % (name, val), ffi), name
    body = re.search(r"pub struct slg_scan_spec \{(.*?)\}", ffi, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", body) == fields
    assert out[-1] == 3 and N.load().slg_abi_version() == 3  # additive: the ABI version stays
    D = plan_lib.slgp_scan_slice_docs()
    assert D % 2048 == 0 and D > 0  # 64 lanes x one bitmap word


def test_scan_py_shapes_the_dictionaries():
    from searchlite_amd import _native as N
    from searchlite_amd.scan import scan_arrays
    a = scan_arrays([MA, CS(filter=3, boost=2.5, node_boost=2.0), RF(7, modifier="log1p", missing=0.5, boost=-2.0),
                     RF(1, modifier="reciprocal", node_boost=3.0), {"match_all": {"filter": 1}}])
    assert a["q_kind"].tolist() == [N.SCAN_MATCH_ALL, N.SCAN_CONSTANT, N.SCAN_RANK_FEATURE, N.SCAN_RANK_FEATURE, 0]
    assert a["q_filter"].tolist() == [-1, 3, -1, -1, 1]
    assert a["q_score"].tolist() == [1.0, 5.0, 1.0, 1.0, 1.0]
    assert a["q_field"].tolist() == [0, 0, 7, 1, 0]
    assert a["q_modifier"].tolist() == [0, 0, N.SCAN_MOD_LOG1P, N.SCAN_MOD_RECIPROCAL, 0]
    assert a["q_missing"].tolist() == [0.0, 0.0, 0.5, 0.0, 0.0] and a["q_boost"].tolist() == [1.0, 1.0, -2.0, 3.0, 1.0]
    with pytest.raises(ValueError):
        scan_arrays([{"match": {"body": "x"}}])
    with pytest.raises(ValueError):
        scan_arrays([{"match_all": {}, "constant_score": {}}])


# ---- refusals ----------------------------------------------------------------------------------------------
def refused(L, code, word, queries, **kw):
    from searchlite_amd import _native as N
    r = plan_scan(L, queries, **kw)
    assert r["rc"] == getattr(N, code) and word in r["msg"], (queries, r["rc"], r["msg"])


def test_null_spec_and_null_arrays(plan_lib):
    refused(plan_lib, "ERR_INVALID", "scan spec is NULL", [MA], spec=(None, None))
    for name in ("q_kind", "q_filter", "q_score", "q_field", "q_modifier", "q_missing", "q_boost"):
        refused(plan_lib, "ERR_INVALID", "is NULL", [MA], spec=spec_of([MA], **{name: None}))
    assert plan_scan(plan_lib, [], spec=spec_of([], q_kind=None))["rc"] == 0  # nq == 0 reads no array


def test_unknown_kind_modifier_and_non_finite_arguments(plan_lib):
    L, F = plan_lib, {0: {}}
    refused(L, "ERR_INVALID", "unknown scan kind in scan query 1", [MA, MA], spec=spec_of([MA, MA], q_kind=[0, 3]))
    refused(L, "ERR_INVALID", "unknown scan kind", [MA], spec=spec_of([MA], q_kind=[-1]))
    refused(L, "ERR_INVALID", "unknown modifier", [RF()], fields=F, spec=spec_of([RF()], q_modifier=[5]))
    refused(L, "ERR_INVALID", "unknown modifier", [RF()], fields=F, spec=spec_of([RF()], q_modifier=[-1]))
    for bad in (np.inf, -np.inf, np.nan):
        refused(L, "ERR_INVALID", "non-finite score", [CS(boost=bad)])
        refused(L, "ERR_INVALID", "non-finite missing", [RF(missing=bad)], fields=F)
        refused(L, "ERR_INVALID", "non-finite boost", [RF(boost=bad)], fields=F)
        # the arguments of another kind are not read
        assert plan_scan(L, [MA], spec=spec_of([MA], q_score=[bad], q_missing=[bad], q_boost=[bad]))["rc"] == 0
        assert plan_scan(L, [CS()], spec=spec_of([CS()], q_missing=[bad], q_boost=[bad]))["rc"] == 0
    refused(L, "ERR_INVALID", "negative filter id", [MA], spec=spec_of([MA], q_filter=[-2]))
    refused(L, "ERR_UNSUPPORTED", "SLG_MAX_K", [MA], k=20002)
    assert plan_scan(L, [MA], k=20001)["rc"] == 0 and plan_scan(L, [MA], k=0)["rc"] == 0
    # an invalid argument is reported before k
    refused(L, "ERR_INVALID", "non-finite score", [CS(boost=np.inf)], k=20002)


def test_filter_and_field_ids_against_the_index(plan_lib):
    L = plan_lib
    fields = {3: {}, 4: dict(keyword=1), 5: dict(has=[1, 0]), 6: dict(non_finite=1)}
    live = [0, 1, 1]  # filter 0 is unknown or incomplete (no bitmap for every segment)
    assert plan_scan(L, [CS(filter=1), RF(3, filter=2)], fields=fields, filter_live=live, q_filter=[2, -1])["rc"] == 0
    refused(L, "ERR_INVALID", "unknown filter id 0 in scan query 1", [MA, CS(filter=0)], filter_live=live)
    refused(L, "ERR_INVALID", "unknown filter id 3", [CS(filter=3)], filter_live=live)
    refused(L, "ERR_INVALID", "unknown filter id 0 in q_filter of query 0", [MA], filter_live=live, q_filter=[0])
    refused(L, "ERR_INVALID", "unknown filter id 7 in q_filter", [MA], filter_live=live, q_filter=[7])
    refused(L, "ERR_INVALID", "unknown filter id -2 in q_filter", [MA], filter_live=live, q_filter=[-2])
    refused(L, "ERR_INVALID", "unknown agg field id 7", [RF(7)], fields=fields)
    refused(L, "ERR_INVALID", "unknown agg field id -1", [RF(-1)], fields=fields)
    refused(L, "ERR_INVALID", "keyword", [RF(4)], fields=fields)
    refused(L, "ERR_INVALID", "no column for segment 1", [RF(5)], fields=fields)
    refused(L, "ERR_UNSUPPORTED", "non-finite", [RF(6)], fields=fields)
    # an invalid argument of a later query is reported before an unsupported column of an earlier one
    refused(L, "ERR_INVALID", "unknown agg field id 7", [RF(6), RF(7)], fields=fields)
    # a match_all or constant_score names no field
    assert plan_scan(L, [MA, CS()], spec=spec_of([MA, CS()], q_field=[99, 4]), fields=fields)["rc"] == 0


# ---- the planned tables ------------------------------------------------------------------------------------
def test_query_records_columns_and_which_kernel(plan_lib):
    f32 = lambda x: int(np.float32(x).view(np.uint32))
    fields = {3: dict(dense=[1, 0]), 8: {}}
    qs = [MA, CS(filter=2, boost=2.5), RF(8, modifier="sqrt", missing=7.0, boost=-2.0), RF(3, filter=0), RF(8, modifier="reciprocal")]
    r = plan_scan(plan_lib, qs, fields=fields, filter_live=[1, 0, 1], q_filter=[-1, 0, -1, 2, -1])
    assert r["rc"] == 0, r["msg"]
    # kind, modifier, filter (0 none, f + 1), col, score, missing, boost, pad
    assert r["queries"].tolist() == [[0, 0, 0, 0, f32(1.0), 0, 0, 0], [1, 0, 3, 0, f32(2.5), 0, 0, 0],
                                     [2, 3, 0, 0, f32(1.0), f32(7.0), f32(-2.0), 0], [2, 0, 1, 1, f32(1.0), 0, f32(1.0), 0],
                                     [2, 4, 0, 0, f32(1.0), 0, f32(1.0), 0]]
    assert r["root"].tolist() == [0, 1, 0, 3, 0] and r["full"] == 0  # none, sqrt, reciprocal: the lean kernel
    addr = lambda owner, s, tag: ((owner + 1) << 32) | (s << 8) | tag
    # columns in order of first use: field 8, then field 3 (segment 0 stored without offsets)
    assert r["cols"].tolist() == [[addr(8, 0, 2), addr(8, 0, 1)], [addr(8, 1, 2), addr(8, 1, 1)],
                                  [0, addr(3, 0, 1)], [addr(3, 1, 2), addr(3, 1, 1)]]
    assert plan_scan(plan_lib, [MA])["root"].tolist() == [0]
    for m, full in (("none", 0), ("sqrt", 0), ("reciprocal", 0), ("log", 1), ("log1p", 1)):
        assert plan_scan(plan_lib, [MA, RF(8, modifier=m)], fields=fields)["full"] == full, m


def test_slice_table_around_the_slice_size(plan_lib):
    D = plan_lib.slgp_scan_slice_docs()
    seg_docs = [1, D - 1, D, D + 1, 0, 2 * D + 5]
    want = [(0, 0, 1), (1, 0, D - 1), (2, 0, D), (3, 0, D), (3, D, 1), (5, 0, D), (5, D, D), (5, 2 * D, 5)]  # seg, first, docs
    fields = {0: dict(has=[1] * 6)}
    for k in (0, 1, 11, D, D + 7):
        for full_regions in (False, True):
            r = plan_scan(plan_lib, [MA, RF(0), CS(boost=3.0)], seg_docs=seg_docs, fields=fields, full_regions=full_regions, k=k)
            assert r["rc"] == 0, r["msg"]
            n = len(want)
            assert r["qrefs"].tolist() == [[0, n], [n, 2 * n], [2 * n, 3 * n]]
            base = 0
            for q in range(3):
                truncated = not full_regions and q != 1  # (a rank_feature query's scores differ: never truncated)
                for i, (seg, first, docs) in enumerate(want):
                    cap = min(docs, k) if truncated else docs
                    assert r["slices"][q * n + i].tolist() == [q, seg, first, docs, cap, 0, 0, 0], (k, full_regions, q, i)
                    assert int(r["cbeg"][q * n + i]) == base
                    base += cap
            assert r["cand_total"] == base
    # no segment, or only empty ones: no slice
    for docs in ([], [0, 0]):
        r = plan_scan(plan_lib, [MA, MA], seg_docs=docs)
        assert r["rc"] == 0 and len(r["slices"]) == 0 and r["qrefs"].tolist() == [[0, 0], [0, 0]] and r["cand_total"] == 0
