"""slg_batch_prepare_fscore / slg_search_batch_fscore argument checks that need no device: the spec is checked before
the index is looked at (a NULL index then fails with SLG_ERR_INVALID and a message, before anything touches a GPU);
field ids, filter ids and the tables the kernel reads are checked through the host planner (plan_fscore: pure host
code); the header, the ctypes binding and the Rust mirror agree on the argument counts and the spec's fields."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {"slg_batch_prepare_fscore": 11, "slg_search_batch_fscore": 17, "slg_batch_fscore_info": 3}

W = lambda w, **kw: dict(kind="weight", weight=w, **kw)
FVF = lambda field=0, **kw: dict(kind="field_value_factor", field=field, **kw)
DECAY = lambda field=0, **kw: dict(dict(kind="decay", field=field, origin=1.0, scale=2.0), **kw)
TWO = [dict(functions=[W(2.0), FVF(modifier="log1p"), DECAY(function="gauss")], min_score=0.5, max_boost=9.0),
       dict(functions=[W(1.0, filter=-1)], score_mode="sum", boost_mode="replace", boost=2.0)]


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


def spec_of(functions=None, **over):
    """the spec of one function_score per query (searcher.fscore_spec; default: TWO); over: fields replaced by an
    array, or None for a NULL pointer -> (N.FscoreSpec, the arrays it points into)"""
    from searchlite_amd import _native as N
    from searchlite_amd.searcher import fscore_spec
    functions = TWO if functions is None else functions
    sp, keep = fscore_spec(functions, len(functions))
    names = [n for n, _ in N.FscoreSpec._fields_]
    for name, v in over.items():
        i = names.index(name)
        if v is not None:
            keep[i] = np.ascontiguousarray(v, dtype=keep[i].dtype)
        setattr(sp, name, None if v is None else keep[i].ctypes.data)
    return sp, keep


def prepare(lib, spec, nq=2, k=11):
    offs = np.zeros(nq + 1, np.uint32)
    return lib.slg_batch_prepare_fscore(None, nq, offs.ctypes.data, None, None, None, None, None,
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


def test_spec_layout_matches_the_header_and_the_rust_mirror(tmp_path, lib):
    import subprocess
    from searchlite_amd import _native as N
    consts = ["SLG_MAX_FSCORE_FUNCS", "SLG_FSCORE_WEIGHT", "SLG_FSCORE_FIELD_VALUE_FACTOR", "SLG_FSCORE_DECAY",
              "SLG_FSCORE_MOD_NONE", "SLG_FSCORE_MOD_LOG", "SLG_FSCORE_MOD_LOG1P", "SLG_FSCORE_MOD_LOG2P",
              "SLG_FSCORE_MOD_SQRT", "SLG_FSCORE_MOD_RECIPROCAL", "SLG_FSCORE_DECAY_EXP", "SLG_FSCORE_DECAY_GAUSS",
              "SLG_FSCORE_DECAY_LINEAR", "SLG_FSCORE_MODE_SUM", "SLG_FSCORE_MODE_MULTIPLY", "SLG_FSCORE_MODE_MAX",
              "SLG_FSCORE_MODE_MIN", "SLG_FSCORE_MODE_AVG", "SLG_FSCORE_BOOST_MULTIPLY", "SLG_FSCORE_BOOST_SUM",
              "SLG_FSCORE_BOOST_REPLACE", "SLG_FSCORE_BOOST_MAX", "SLG_FSCORE_BOOST_MIN", "SLG_FSCORE_HAS_MAX_BOOST",
              "SLG_FSCORE_HAS_MIN_SCORE"]
    fields = [n for n, _ in N.FscoreSpec._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(slg_fscore_spec));\n' +
                   "".join('  printf(" %%zu", offsetof(slg_fscore_spec, %s));\n' % f for f in fields) +
                   "".join('  printf(" %%d", (int)%s);\n' % c for c in consts) + '  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert out[0] == C.sizeof(N.FscoreSpec)
    assert out[1:1 + len(fields)] == [getattr(N.FscoreSpec, f).offset for f in fields]
    values = dict(zip(consts, out[1 + len(fields):]))
    assert values["SLG_MAX_FSCORE_FUNCS"] == N.MAX_FSCORE_FUNCS == 8
    ffi = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    for name, val in values.items():
        assert getattr(N, name[4:]) == val, name
        assert re.search(r"pub const %s: \w+ = %d;" % (name, val), ffi), name
    body = re.search(r"pub struct slg_fscore_spec \{(.*?)\}", ffi, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", body) == fields
    assert lib.slg_abi_version() == 3


def test_null_spec_and_null_index(lib):
    rejected(lib, None, "ERR_INVALID", "fscore spec is NULL")
    rejected(lib, spec_of(), "ERR_INVALID", "index is NULL")  # a valid spec: the index is looked at next
    rejected(lib, spec_of([]), "ERR_INVALID", "index is NULL", nq=0)
    rejected(lib, spec_of([None, None]), "ERR_INVALID", "index is NULL")  # no query has work
    rejected(lib, spec_of([dict(functions=[W(1.0)] * 8), None]), "ERR_INVALID", "index is NULL")  # 8 functions fit


@pytest.mark.parametrize("name", ["q_fn_offsets", "q_score_mode", "q_boost_mode", "q_flags", "q_boost", "q_max_boost",
                                  "q_min_score", "f_kind", "f_field", "f_filter", "f_weight", "f_modifier", "f_decay_fn",
                                  "f_missing", "f_origin", "f_scale", "f_offset", "f_decay"])
def test_null_arrays(lib, name):
    rejected(lib, spec_of(**{name: None}), "ERR_INVALID", name if name.startswith("q_") else "f_ array")


def test_arrays_a_spec_does_not_need(lib):
    none = [None, dict(boost=2.0)]
    f_arrays = {n: None for n in ("f_kind", "f_field", "f_filter", "f_weight", "f_modifier", "f_decay_fn", "f_missing",
                                  "f_origin", "f_scale", "f_offset", "f_decay")}
    rejected(lib, spec_of(none, q_max_boost=None, q_min_score=None, **f_arrays), "ERR_INVALID", "index is NULL")


def test_offsets_that_decrease(lib):
    rejected(lib, spec_of(q_fn_offsets=np.array([0, 3, 2], np.uint32)), "ERR_INVALID", "q_fn_offsets not monotone")


@pytest.mark.parametrize("over,word", [
    (dict(f_kind=[0, 3, 2, 0]), "unknown function kind"), (dict(f_kind=[-1, 1, 2, 0]), "unknown function kind"),
    (dict(q_score_mode=[5, 0]), "unknown score mode"), (dict(q_score_mode=[0, -1]), "unknown score mode"),
    (dict(q_boost_mode=[0, 5]), "unknown boost mode"), (dict(q_flags=[4, 0]), "unknown flag"),
    (dict(f_modifier=[0, 6, 0, 0]), "unknown modifier"), (dict(f_modifier=[0, -1, 0, 0]), "unknown modifier"),
    (dict(f_decay_fn=[0, 0, 3, 0]), "unknown decay function"),
    (dict(f_weight=[np.inf, 1, 1, 1]), "non-finite weight"), (dict(f_weight=[1, np.nan, 1, 1]), "non-finite factor"),
    (dict(f_scale=[1, 1, np.inf, 1]), "scale must be finite"), (dict(f_scale=[1, 1, np.nan, 1]), "scale must be finite"),
    (dict(f_scale=[1, 1, 0.0, 1]), "scale must be > 0"), (dict(f_scale=[1, 1, -2.0, 1]), "scale must be > 0"),
    (dict(f_decay=[.5, .5, 0.0, .5]), "outside (0, 1]"), (dict(f_decay=[.5, .5, 1.0000001, .5]), "outside (0, 1]"),
    (dict(f_decay=[.5, .5, np.nan, .5]), "outside (0, 1]"), (dict(f_filter=[-2, -1, -1, -1]), "filter id"),
])
def test_invalid_values(lib, over, word):
    rejected(lib, spec_of(**over), "ERR_INVALID", word)


def test_values_only_their_kind_reads(lib):
    # a weight's scale / decay / modifier and a decay's weight are not looked at; decay = 1 is inside (0, 1]
    rejected(lib, spec_of(f_scale=[-1, -1, 2.0, np.nan], f_decay=[7, 7, 1.0, 7], f_modifier=[9, 0, 9, 9],
                          f_decay_fn=[9, 9, 1, 9], f_weight=[1, 1, np.nan, 1]), "ERR_INVALID", "index is NULL")


def test_function_limit(lib):
    nine = dict(functions=[W(1.0)] * 9)
    rejected(lib, spec_of([None, nine]), "ERR_UNSUPPORTED", "SLG_MAX_FSCORE_FUNCS")
    # an invalid argument is reported before an unsupported one
    rejected(lib, spec_of([nine, dict(functions=[W(np.inf)])]), "ERR_INVALID", "non-finite weight")


def test_one_call_form_null_arguments(lib):
    from searchlite_amd import _native as N
    sp, keep = spec_of()
    args = (None, None, None, None, None, None)
    assert lib.slg_search_batch_fscore(None, 0, None, None, None, None, None, None, C.addressof(sp), 11, 1, *args) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error()
    assert lib.slg_search_batch_fscore(None, 0, None, None, None, None, None, None, None, 11, 1, *args) == N.ERR_INVALID
    assert b"fscore spec is NULL" in lib.slg_last_error()
    assert lib.slg_batch_fscore_info(None, None, None) == N.ERR_INVALID


# ---- the host planner: ids against the registered fields and filters, and the tables the kernel reads ----
class Field(C.Structure):
    _fields_ = [("id", C.c_int32), ("keyword", C.c_uint32), ("non_finite", C.c_uint32), ("seg_has", C.c_void_p),
                ("seg_dense", C.c_void_p)]


def plan_fscore(functions, fields, filter_live=(), n_segs=2):
    """fields: {id: dict(keyword=, non_finite=, has=[per segment], dense=[per segment])} -> (code, message, FscoreQuery
    words [nq, 8], FscoreFn records, column addresses [n, 2], filter addresses, (n_work, full)) of slgplan::plan_fscore"""
    from searchlite_amd import build
    L = C.CDLL(build.build_plan_lib())
    L.slgp_plan_fscore.restype = C.c_int
    keep, arr = [], (Field * max(len(fields), 1))()
    for i, (fid, f) in enumerate(fields.items()):
        has = np.array(f.get("has", [1] * n_segs), np.uint8)
        dense = np.array(f.get("dense", [0] * n_segs), np.uint8)
        keep += [has, dense]
        arr[i] = Field(fid, int(f.get("keyword", 0)), int(f.get("non_finite", 0)), has.ctypes.data, dense.ctypes.data)
    live = np.array(list(filter_live) + [0], np.uint8)
    sp, keep2 = spec_of(functions)
    nq = len(functions)
    fn_dt = np.dtype([("kinds", "<u4"), ("col", "<u4"), ("filter", "<u4"), ("weight", "<f4"), ("missing", "<f8"),
                      ("origin", "<f8"), ("scale", "<f8"), ("offset", "<f8"), ("decay", "<f8"), ("pad", "<u4", 2)])
    assert fn_dt.itemsize == 64
    qw, fns = np.zeros((max(nq, 1), 8), np.uint32), np.zeros(64, fn_dt)
    cols, flt = np.zeros((64, 2), np.uint64), np.zeros(64, np.uint64)
    counts, err = (C.c_uint32 * 5)(), C.create_string_buffer(256)
    rc = L.slgp_plan_fscore(arr, len(fields), C.c_void_p(live.ctypes.data), len(filter_live), n_segs, nq, C.byref(sp),
                            C.c_void_p(qw.ctypes.data), C.c_void_p(fns.ctypes.data), 64, C.c_void_p(cols.ctypes.data), 64,
                            C.c_void_p(flt.ctypes.data), 64, counts, err, 256)
    return rc, err.value.decode(), qw[:nq], fns[:counts[0]], cols[:counts[1]], flt[:counts[2]], (counts[3], counts[4])


def test_ids_against_the_registered_fields_and_filters():
    from searchlite_amd import _native as N
    fields = {3: {}, 4: dict(keyword=1), 5: dict(has=[1, 0]), 6: dict(non_finite=1)}
    one = lambda fn: [dict(functions=[fn])]
    assert plan_fscore(one(FVF(3, filter=1)), fields, [0, 1])[0] == N.OK
    assert plan_fscore(one(W(1.0, field=99)), fields)[0] == N.OK  # a weight names no field
    for fn, code, word in ((FVF(7), N.ERR_INVALID, "unknown agg field id 7"), (DECAY(-1), N.ERR_INVALID, "unknown agg field"),
                           (FVF(4), N.ERR_INVALID, "keyword"), (DECAY(5), N.ERR_INVALID, "no column for segment 1"),
                           (FVF(6), N.ERR_UNSUPPORTED, "non-finite"), (W(1.0, filter=0), N.ERR_INVALID, "unknown filter id 0"),
                           (FVF(3, filter=2), N.ERR_INVALID, "unknown filter id 2")):
        rc, msg = plan_fscore(one(fn), fields, [0, 1])[:2]
        assert rc == code and word in msg, (fn, rc, msg)
    # an invalid argument of a later query is reported before an unsupported column of an earlier one
    rc, msg = plan_fscore([dict(functions=[FVF(6)]), dict(functions=[FVF(7)])], fields)[:2]
    assert rc == N.ERR_INVALID and "unknown agg field id 7" in msg


def test_tables_of_plan_fscore():
    from searchlite_amd import _native as N
    fields = {3: dict(dense=[1, 0]), 8: {}}
    functions = [dict(functions=[W(2.5, filter=2), FVF(8, factor=0.5, modifier="sqrt", missing=7.0),
                                 DECAY(3, function="linear", offset=0.25, decay=0.75, filter=0)],
                      score_mode="avg", boost_mode="max", max_boost=9.0, boost=-2.0),
                 None,
                 dict(min_score=0.5),
                 dict(functions=[FVF(8, filter=2)], score_mode="sum", boost_mode="replace")]
    rc, msg, qw, fns, cols, flt, (n_work, full) = plan_fscore(functions, fields, [1, 0, 1])
    assert rc == N.OK, msg
    f32 = lambda x: int(np.float32(x).view(np.uint32))
    # fn_begin, n_fns, modes (score | boost << 8 | flags << 16), work, max_boost, min_score, boost, pad
    assert qw.tolist() == [[0, 3, 4 | 3 << 8 | 1 << 16, 1, f32(9.0), 0, f32(-2.0), 0],
                           [3, 0, 1 | 0 << 8, 0, 0, 0, f32(1.0), 0],
                           [3, 0, 1 | 0 << 8 | 2 << 16, 1, 0, f32(0.5), f32(1.0), 0],
                           [3, 1, 0 | 2 << 8, 1, 0, 0, f32(1.0), 0]]
    assert (n_work, full) == (3, 0)  # weight, sqrt, linear and none: the lean kernel
    assert fns["kinds"].tolist() == [0, 1 | 4 << 8, 2 | 2 << 16, 1]
    assert fns["col"].tolist() == [0, 0, 1, 0] and fns["filter"].tolist() == [1, 0, 2, 1]  # rows in order of first use
    assert fns["weight"].tolist() == [2.5, 0.5, 1.0, 1.0] and fns["missing"].tolist() == [0.0, 7.0, 0.0, 0.0]
    assert (fns["origin"][2], fns["scale"][2], fns["offset"][2], fns["decay"][2]) == (1.0, 2.0, 0.25, 0.75)
    addr = lambda owner, s, tag: ((owner + 1) << 32) | (s << 8) | tag
    # columns: field 8 first, then field 3 (segment 0 stored without offsets); filters: 2 first, then 0
    assert cols.tolist() == [[addr(8, 0, 2), addr(8, 0, 1)], [addr(8, 1, 2), addr(8, 1, 1)],
                             [0, addr(3, 0, 1)], [addr(3, 1, 2), addr(3, 1, 1)]]
    assert flt.tolist() == [addr(2, 0, 3), addr(2, 1, 3), addr(0, 0, 3), addr(0, 1, 3)]


@pytest.mark.parametrize("fn,full", [(W(1.0), 0), (FVF(0), 0), (FVF(0, modifier="sqrt"), 0), (FVF(0, modifier="reciprocal"), 0),
                                     (DECAY(0, function="linear"), 0), (FVF(0, modifier="log"), 1),
                                     (FVF(0, modifier="log1p"), 1), (FVF(0, modifier="log2p"), 1),
                                     (DECAY(0, function="exp"), 1), (DECAY(0, function="gauss"), 1)])
def test_which_kernel_a_batch_needs(fn, full):
    rc, msg, *_, (n_work, got) = plan_fscore([dict(functions=[W(1.0)]), dict(functions=[fn])], {0: {}})
    assert rc == 0 and (n_work, got) == (2, full), msg
