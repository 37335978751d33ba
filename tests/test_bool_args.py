"""slg_batch_prepare_bool / slg_search_batch_bool argument checks that need no device: the spec is checked before
the index is looked at, a NULL index fails with SLG_ERR_INVALID and a message, before anything touches a GPU; the
term ids and the clause tables are checked through the host planner (plan_bool: pure host code); the header, the
ctypes binding and the Rust mirror agree on the argument counts and the spec's fields."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import bool_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {"slg_batch_prepare_bool": 11, "slg_search_batch_bool": 17}


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


def spec_of(queries=None, n_segs=1, **over):
    """the spec of `queries` (bool_ref.clauses_of; default: two queries of a MUST, a SHOULD and a MUST_NOT group);
    over: fields replaced (None: a NULL pointer) -> (N.BoolSpec, the arrays it points into)"""
    from searchlite_amd import _native as N
    if queries is None:
        queries = [([(B.MUST, [0]), (B.SHOULD, [1, 2]), (B.MUST_NOT, [3])], 1)] * 2
    cl = B.clauses_of(queries, n_segs)
    a = dict(c_offsets=cl["c_offsets"], c_term_ids=cl["c_terms"], c_group=cl["c_group"], g_offsets=cl["g_offsets"],
             g_kind=cl["g_kind"], q_min_should=cl["q_min_should"])
    a.update(over)
    a = {n: None if v is None else np.ascontiguousarray(v) for n, v in a.items()}
    return N.BoolSpec(*[None if a[n] is None else a[n].ctypes.data for n, _ in N.BoolSpec._fields_]), a


def prepare(lib, spec, nq=2, k=11, plans=None):
    offs = np.zeros(nq + 1, np.uint32)
    return lib.slg_batch_prepare_bool(None, nq, offs.ctypes.data, None, None, None if plans is None else C.addressof(plans),
                                      None, None, None if spec is None else C.addressof(spec), k, 1)


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
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %u %u %d %d %d\\n", sizeof(slg_bool_spec), offsetof(slg_bool_spec, g_offsets),\n'
                   '         offsetof(slg_bool_spec, q_min_should), SLG_MAX_BOOL_GROUPS, SLG_MAX_BOOL_TERMS,\n'
                   '         SLG_BOOL_MUST, SLG_BOOL_SHOULD, SLG_BOOL_MUST_NOT);\n  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_goff, o_ms, max_g, max_t, must, should, must_not = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(N.BoolSpec)
    assert o_goff == N.BoolSpec.g_offsets.offset and o_ms == N.BoolSpec.q_min_should.offset
    assert max_g == N.MAX_BOOL_GROUPS == 32 and max_t == N.MAX_BOOL_TERMS == 64
    assert (must, should, must_not) == (N.BOOL_MUST, N.BOOL_SHOULD, N.BOOL_MUST_NOT) == (B.MUST, B.SHOULD, B.MUST_NOT)
    ffi = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    body = re.search(r"pub struct slg_bool_spec \{(.*?)\}", ffi, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", body) == [n for n, _ in N.BoolSpec._fields_]
    for name, val in (("SLG_MAX_BOOL_GROUPS", 32), ("SLG_MAX_BOOL_TERMS", 64), ("SLG_BOOL_MUST_NOT", 2)):
        assert re.search(r"pub const %s: \w+ = %d;" % (name, val), ffi), name
    assert lib_abi_version() == 3


def lib_abi_version():
    from searchlite_amd import _native
    return _native.load().slg_abi_version()


def test_null_spec_and_null_index(lib):
    rejected(lib, None, "ERR_INVALID", "bool spec is NULL")
    rejected(lib, spec_of(), "ERR_INVALID", "index is NULL")  # a valid spec: the index is looked at next
    rejected(lib, spec_of([]), "ERR_INVALID", "index is NULL", nq=0)
    rejected(lib, spec_of([([], 0), ([], 3)]), "ERR_INVALID", "index is NULL")  # no query has a clause table


def test_null_arrays(lib):
    rejected(lib, spec_of(c_offsets=None), "ERR_INVALID", "c_offsets")
    rejected(lib, spec_of(g_offsets=None), "ERR_INVALID", "g_offsets")
    rejected(lib, spec_of(c_term_ids=None), "ERR_INVALID", "c_term_ids")
    rejected(lib, spec_of(c_group=None), "ERR_INVALID", "c_group")
    rejected(lib, spec_of(g_kind=None), "ERR_INVALID", "g_kind")
    rejected(lib, spec_of(q_min_should=None), "ERR_INVALID", "index is NULL")  # NULL: 0 for every query
    # a spec without a single term or group needs none of the three
    rejected(lib, spec_of([([], 0), ([], 0)], c_term_ids=None, c_group=None, g_kind=None), "ERR_INVALID", "index is NULL")


def test_offsets_that_decrease(lib):
    rejected(lib, spec_of(c_offsets=np.array([0, 5, 4], np.uint32)), "ERR_INVALID", "c_offsets not monotone")
    rejected(lib, spec_of(g_offsets=np.array([0, 4, 3], np.uint32)), "ERR_INVALID", "g_offsets not monotone")


def test_bad_groups(lib):
    good = np.array([0, 1, 1, 2, 0, 1, 1, 2], np.uint32)
    rejected(lib, spec_of(c_group=good), "ERR_INVALID", "index is NULL")
    rejected(lib, spec_of(c_group=np.array([0, 1, 0, 2, 0, 1, 1, 2], np.uint32)), "ERR_INVALID", "decreases or skips")
    rejected(lib, spec_of(c_group=np.array([0, 0, 2, 2, 0, 1, 1, 2], np.uint32)), "ERR_INVALID", "decreases or skips")
    rejected(lib, spec_of(c_group=np.array([1, 1, 1, 2, 0, 1, 1, 2], np.uint32)), "ERR_INVALID", "decreases or skips")
    rejected(lib, spec_of(c_group=np.array([0, 1, 2, 3, 0, 1, 1, 2], np.uint32)), "ERR_INVALID", "does not have")
    # a group without a term: the last group, and every group of a query without terms
    rejected(lib, spec_of(c_group=np.array([0, 1, 1, 1, 0, 1, 1, 2], np.uint32)), "ERR_INVALID", "group without a term")
    rejected(lib, spec_of(c_offsets=np.array([0, 0, 4], np.uint32), c_group=np.array([0, 1, 1, 2], np.uint32),
                          c_term_ids=np.zeros(4, np.uint32)), "ERR_INVALID", "group without a term")


@pytest.mark.parametrize("kind", [-1, 3, 100])
def test_unknown_kind(lib, kind):
    rejected(lib, spec_of(g_kind=np.array([0, 1, 2, 0, kind, 2], np.int32)), "ERR_INVALID", "clause kind")


def test_min_match_in_the_plans(lib):
    from searchlite_amd import _native as N
    for mm, ok in (([0, 1], True), ([1, 2], False), ([5, 0], False)):
        arr = np.array(mm, np.uint32)
        plans = N.ScorePlans()
        plans.q_min_match = arr.ctypes.data
        if ok:
            rejected(lib, spec_of(), "ERR_INVALID", "index is NULL", plans=plans)
        else:
            rejected(lib, spec_of(), "ERR_INVALID", "q_min_match", plans=plans)


def test_group_and_term_limits(lib):
    from searchlite_amd import _native as N
    G, T = N.MAX_BOOL_GROUPS, N.MAX_BOOL_TERMS
    rejected(lib, spec_of([([(B.SHOULD, [g, g + 1]) for g in range(G)], 3)] * 2), "ERR_INVALID", "index is NULL")  # 32 / 64
    rejected(lib, spec_of([([(B.SHOULD, [g]) for g in range(G + 1)], 3), ([], 0)]), "ERR_UNSUPPORTED", "SLG_MAX_BOOL_GROUPS")
    rejected(lib, spec_of([([], 0), ([(B.MUST, list(range(T + 1)))], 0)]), "ERR_UNSUPPORTED", "SLG_MAX_BOOL_TERMS")
    # an invalid argument is reported before an unsupported one
    rejected(lib, spec_of([([(B.SHOULD, [g]) for g in range(G + 1)], 3), ([(7, [0])], 0)]), "ERR_INVALID", "clause kind")
    # min_should above the number of SHOULD groups is valid (it matches nothing)
    rejected(lib, spec_of([([(B.SHOULD, [0])], 9)] * 2), "ERR_INVALID", "index is NULL")


def test_one_call_form_null_arguments(lib):
    from searchlite_amd import _native as N
    sp, keep = spec_of()
    args = (None, None, None, None, None, None)
    assert lib.slg_search_batch_bool(None, 0, None, None, None, None, None, None, C.addressof(sp), 11, 1, *args) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error()
    assert lib.slg_search_batch_bool(None, 0, None, None, None, None, None, None, None, 11, 1, *args) == N.ERR_INVALID
    assert b"bool spec is NULL" in lib.slg_last_error()


# ---- the host planner: term ids against the segments' dictionaries, and the tables the kernel reads ----
class Seg(C.Structure):
    _fields_ = [("n_docs", C.c_uint32), ("n_terms", C.c_uint32), ("term_offsets", C.c_void_p), ("champ", C.c_void_p)]


def plan_bool(queries, seg_offsets, plans=None):
    """-> (code, message, BoolQuery words [nq, 8], BoolTerm words [n, 4]) of slgplan::plan_bool over segments with
    the given term_offsets"""
    from searchlite_amd import build
    L = C.CDLL(build.build_plan_lib())
    L.slgp_plan_bool.restype = C.c_int
    offs = [np.asarray(o, np.uint64) for o in seg_offsets]
    segs = (Seg * len(offs))(*[Seg(100, len(o) - 1, o.ctypes.data, None) for o in offs])
    sp, keep = spec_of(queries, len(offs))
    nq = len(queries)
    qw, tw = np.zeros((max(nq, 1), 8), np.uint32), np.zeros((4096, 4), np.uint32)
    n, err = C.c_uint32(), C.create_string_buffer(256)
    rc = L.slgp_plan_bool(segs, len(offs), nq, C.byref(sp), None if plans is None else C.byref(plans),
                          C.c_void_p(qw.ctypes.data), C.c_void_p(tw.ctypes.data), 4096, C.byref(n), err, 256)
    return rc, err.value.decode(), qw[:nq], tw[:n.value]


def test_term_id_beyond_a_segments_dictionary():
    from searchlite_amd import _native as N
    offs = [[0, 3, 3, 10], [0, 5]]  # 3 terms, 1 term
    q = lambda t: [([(B.MUST, [t])], 0)]
    assert plan_bool(q((2, 0)), offs)[0] == N.OK
    assert plan_bool(q((2, N.NO_TERM)), offs)[0] == N.OK
    for bad in ((3, 0), (0, 1), (0xFFFFFFFE, 0)):
        rc, msg, _, _ = plan_bool(q(bad), offs)
        assert rc == N.ERR_INVALID and "term id out of range" in msg, (bad, rc, msg)


def test_tables_of_plan_bool():
    """masks, counts and the row order MUST, MUST_NOT, SHOULD; offsets in the padded layout (+ 64 per term); an
    absent term and an empty list have df 0; a query without groups has no terms and its min_should is dropped"""
    from searchlite_amd import _native as N
    offs = [[0, 3, 3, 10], [0, 5, 9]]
    queries = [([(B.SHOULD, [(2, 1)]), (B.MUST, [(0, 0), (1, N.NO_TERM)]), (B.MUST_NOT, [(2, N.NO_TERM)])], 1),
               ([], 7),
               ([(B.MUST_NOT, [(1, 1)])], 0)]
    rc, msg, qw, tw = plan_bool(queries, offs)
    assert rc == N.OK, msg
    # term_begin, n_terms, must, must_not, should, min_should, n_must, n_must_not
    assert qw.tolist() == [[0, 4, 0b010, 0b100, 0b001, 1, 2, 1], [4, 0, 0, 0, 0, 0, 0, 0], [4, 1, 0, 1, 0, 0, 0, 1]]
    rows = [(int(lo) | (int(hi) << 32), int(df), int(g)) for lo, hi, df, g in tw]
    assert rows[0:4] == [(0, 3, 1), (3 + 64, 0, 1), (3 + 128, 7, 2), (3 + 128, 7, 0)]      # query 0, segment 0
    assert rows[4:8] == [(0, 5, 1), (0, 0, 1), (0, 0, 2), (5 + 64, 4, 0)]                  # query 0, segment 1
    assert rows[8:] == [(3 + 64, 0, 0), (5 + 64, 4, 0)]                                    # query 2, both segments
    assert len(rows) == 10
