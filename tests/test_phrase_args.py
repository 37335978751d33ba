"""slg_batch_prepare_phrase / slg_search_batch_phrase / slg_index_set_positions argument checks that need no
device: the specs are checked before the index is looked at (a NULL index then fails with SLG_ERR_INVALID and a
message, before anything touches a GPU); the term ids, the planned tables and the position checks go through the
host planner (check_phrase / plan_phrase / check_positions: pure host code); the header, the ctypes binding and
the Rust mirror agree on the argument counts and the spec's fields."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import bool_ref as B
from tests import phrase_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {"slg_batch_prepare_phrase": 12, "slg_search_batch_phrase": 18, "slg_index_set_positions": 4}
MUST, SHOULD, MUST_NOT = P.MUST, P.SHOULD, P.MUST_NOT


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


def default_queries():
    """two queries of a MUST phrase of two variants with slop 1 and a SHOULD one-term phrase"""
    return [([(MUST, 1, [[0, 1], [2, 3, 4]]), (SHOULD, 0, [[5]])], 1)] * 2


def spec_of(queries=None, n_segs=1, **over):
    """the phrase spec of `queries` (phrase_ref.phrases_of); over: fields replaced (None: a NULL pointer)
    -> (N.PhraseSpec, the arrays it points into)"""
    from searchlite_amd import _native as N
    ph = P.phrases_of(default_queries() if queries is None else queries, n_segs)
    a = dict(p_offsets=ph["p_offsets"], p_kind=ph["p_kind"], p_slop=ph["p_slop"], v_offsets=ph["v_offsets"],
             t_offsets=ph["t_offsets"], t_term_ids=ph["t_terms"], q_min_should=ph["q_min_should"])
    a.update(over)
    a = {n: None if v is None else np.ascontiguousarray(v) for n, v in a.items()}
    return N.PhraseSpec(*[None if a[n] is None else a[n].ctypes.data for n, _ in N.PhraseSpec._fields_]), a


def bool_spec_of(queries, n_segs=1, min_should=False):
    from searchlite_amd import _native as N
    cl = B.clauses_of(queries, n_segs)
    a = [cl["c_offsets"], cl["c_terms"], cl["c_group"], cl["g_offsets"], cl["g_kind"], cl["q_min_should"] if min_should else None]
    a = [None if v is None else np.ascontiguousarray(v) for v in a]
    return N.BoolSpec(*[None if v is None else v.ctypes.data for v in a]), a


def prepare(lib, spec, nq=2, k=11, plans=None, boolean=None):
    offs = np.zeros(nq + 1, np.uint32)
    return lib.slg_batch_prepare_phrase(None, nq, offs.ctypes.data, None, None, None if plans is None else C.addressof(plans),
                                        None, None, None if boolean is None else C.addressof(boolean),
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


def test_spec_layout_matches_the_header_and_the_rust_mirror(lib, tmp_path):
    import subprocess
    from searchlite_amd import _native as N
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %u %u %u %u\\n", sizeof(slg_phrase_spec), offsetof(slg_phrase_spec, v_offsets),\n'
                   '         offsetof(slg_phrase_spec, q_min_should), SLG_MAX_PHRASE_TERMS, SLG_MAX_PHRASE_VARIANTS,\n'
                   '         SLG_MAX_PHRASE_QUERY_TERMS, SLG_MAX_PHRASE_SLOP);\n  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_v, o_ms, max_t, max_v, max_q, max_slop = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(N.PhraseSpec)
    assert o_v == N.PhraseSpec.v_offsets.offset and o_ms == N.PhraseSpec.q_min_should.offset
    assert (max_t, max_v, max_q) == (N.MAX_PHRASE_TERMS, N.MAX_PHRASE_VARIANTS, N.MAX_PHRASE_QUERY_TERMS) == (8, 8, 64)
    assert max_slop == N.MAX_PHRASE_SLOP == 2 ** 31 - 1 - 8
    ffi = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    body = re.search(r"pub struct slg_phrase_spec \{(.*?)\}", ffi, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", body) == [n for n, _ in N.PhraseSpec._fields_]
    for name, val in (("SLG_MAX_PHRASE_TERMS", 8), ("SLG_MAX_PHRASE_VARIANTS", 8), ("SLG_MAX_PHRASE_QUERY_TERMS", 64),
                      ("SLG_MAX_PHRASE_SLOP", 2 ** 31 - 1 - 8)):
        assert re.search(r"pub const %s: \w+ = %d;" % (name, val), ffi), name
    assert lib.slg_abi_version() == 3


def test_null_spec_and_null_index(lib):
    rejected(lib, None, "ERR_INVALID", "phrase spec is NULL")
    rejected(lib, spec_of(), "ERR_INVALID", "index is NULL")  # a valid spec: the index is looked at next
    rejected(lib, spec_of([]), "ERR_INVALID", "index is NULL", nq=0)
    rejected(lib, spec_of([([], 0), ([], 3)]), "ERR_INVALID", "index is NULL")  # no query has a group
    rejected(lib, spec_of([([(MUST, 0, [])], 0)] * 2), "ERR_INVALID", "index is NULL")  # a group with zero variants
    assert lib.slg_index_set_positions(None, 0, None, None) < 0 and b"index is NULL" in lib.slg_last_error()


def test_null_arrays(lib):
    for name in ("p_offsets", "p_kind", "p_slop", "v_offsets", "t_offsets", "t_term_ids"):
        rejected(lib, spec_of(**{name: None}), "ERR_INVALID", name)
    rejected(lib, spec_of(q_min_should=None), "ERR_INVALID", "index is NULL")  # NULL: 0 for every query
    # a spec without a phrase needs none of the arrays behind p_offsets
    rejected(lib, spec_of([([], 0), ([], 0)], p_kind=None, p_slop=None, v_offsets=None, t_offsets=None, t_term_ids=None),
             "ERR_INVALID", "index is NULL")


def test_offsets_that_decrease_and_empty_variants(lib):
    rejected(lib, spec_of(p_offsets=np.array([0, 2, 1], np.uint32)), "ERR_INVALID", "p_offsets not monotone")
    rejected(lib, spec_of(v_offsets=np.array([0, 2, 1, 5, 6], np.uint32)), "ERR_INVALID", "v_offsets not monotone")
    rejected(lib, spec_of(t_offsets=np.array([0, 2, 5, 4, 8, 11, 12], np.uint32)), "ERR_INVALID", "t_offsets not monotone")
    rejected(lib, spec_of(t_offsets=np.array([0, 2, 2, 6, 8, 11, 12], np.uint32)), "ERR_INVALID", "variant without a term")
    rejected(lib, spec_of([([(MUST, 0, [[]])], 0)] * 2), "ERR_INVALID", "variant without a term")


@pytest.mark.parametrize("kind", [-1, 3, 100])
def test_unknown_kind(lib, kind):
    rejected(lib, spec_of(p_kind=np.array([0, 1, kind, 1], np.int32)), "ERR_INVALID", "phrase kind")


def test_min_match_in_the_plans_and_min_should_in_the_bool_spec(lib):
    from searchlite_amd import _native as N
    for mm, ok in (([0, 1], True), ([1, 2], False), ([5, 0], False)):
        arr = np.array(mm, np.uint32)
        plans = N.ScorePlans()
        plans.q_min_match = arr.ctypes.data
        rejected(lib, spec_of(), "ERR_INVALID", "index is NULL" if ok else "q_min_match", plans=plans)
    tg = [([(MUST, [0]), (SHOULD, [1, 2])], 1)] * 2
    bs, keep = bool_spec_of(tg)
    rejected(lib, spec_of(), "ERR_INVALID", "index is NULL", boolean=bs)
    bs, keep = bool_spec_of(tg, min_should=True)
    rejected(lib, spec_of(), "ERR_INVALID", "q_min_should", boolean=bs)
    bs, keep = bool_spec_of([([(7, [0])], 0)] * 2)  # whatever a bool batch refuses in the bool spec
    rejected(lib, spec_of(), "ERR_INVALID", "clause kind", boolean=bs)


def test_limits(lib):
    from searchlite_amd import _native as N
    ok = [([(MUST, N.MAX_PHRASE_SLOP, [list(range(8))] * 8)], 0)] * 2  # 8 terms, 8 variants, 64 terms, the top slop
    rejected(lib, spec_of(ok), "ERR_INVALID", "index is NULL")
    rejected(lib, spec_of([([(MUST, 0, [list(range(9))])], 0), ([], 0)]), "ERR_UNSUPPORTED", "SLG_MAX_PHRASE_TERMS")
    rejected(lib, spec_of([([], 0), ([(MUST, 0, [[1]] * 9)], 0)]), "ERR_UNSUPPORTED", "SLG_MAX_PHRASE_VARIANTS")
    rejected(lib, spec_of([([(MUST, 0, [list(range(8))] * 8), (SHOULD, 0, [[1]])], 0)] * 2), "ERR_UNSUPPORTED",
             "SLG_MAX_PHRASE_QUERY_TERMS")
    rejected(lib, spec_of([([(MUST, N.MAX_PHRASE_SLOP + 1, [[1, 2]])], 0)] * 2), "ERR_UNSUPPORTED", "SLG_MAX_PHRASE_SLOP")
    many = lambda n: [([(SHOULD, 0, [[g % 8]]) for g in range(n)], 3)] * 2
    rejected(lib, spec_of(many(32)), "ERR_INVALID", "index is NULL")
    rejected(lib, spec_of(many(33)), "ERR_UNSUPPORTED", "SLG_MAX_BOOL_GROUPS")
    bs, keep = bool_spec_of([([(SHOULD, [g]) for g in range(12)], 0)] * 2)  # term groups count too
    rejected(lib, spec_of(many(20)), "ERR_INVALID", "index is NULL", boolean=bs)
    rejected(lib, spec_of(many(21)), "ERR_UNSUPPORTED", "SLG_MAX_BOOL_GROUPS", boolean=bs)
    # an invalid argument is reported before an unsupported one
    rejected(lib, spec_of([([(MUST, 0, [list(range(9))])], 0), ([(9, 0, [[1]])], 0)]), "ERR_INVALID", "phrase kind")
    # min_should above the number of SHOULD groups is valid (it matches nothing)
    rejected(lib, spec_of([([(SHOULD, 0, [[0]])], 9)] * 2), "ERR_INVALID", "index is NULL")


def test_one_call_form_null_arguments(lib):
    from searchlite_amd import _native as N
    sp, keep = spec_of()
    args = (None, None, None, None, None, None)
    assert lib.slg_search_batch_phrase(None, 0, None, None, None, None, None, None, None, C.addressof(sp), 11, 1, *args) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error()
    assert lib.slg_search_batch_phrase(None, 0, None, None, None, None, None, None, None, None, 11, 1, *args) == N.ERR_INVALID
    assert b"phrase spec is NULL" in lib.slg_last_error()


# ---- the host planner: term ids against the segments' dictionaries, the tables the kernel reads, positions ----
class Seg(C.Structure):
    _fields_ = [("n_docs", C.c_uint32), ("n_terms", C.c_uint32), ("term_offsets", C.c_void_p), ("champ", C.c_void_p)]


def plan_lib():
    from searchlite_amd import build
    return C.CDLL(build.build_plan_lib())


def plan_phrase(queries, seg_offsets, term_groups=None, has_pos=None):
    """-> (code, message, BoolQuery words [nq, 8], PhraseQuery words [nq, 8], PhraseVar words [n, 4], PhraseTerm
    words [n, 6], BoolTerm words [n, 4]) of slgplan::plan_phrase over segments with the given term_offsets"""
    L = plan_lib()
    L.slgp_plan_phrase.restype = C.c_int
    offs = [np.asarray(o, np.uint64) for o in seg_offsets]
    segs = (Seg * len(offs))(*[Seg(100, len(o) - 1, o.ctypes.data, None) for o in offs])
    sp, keep = spec_of(queries, len(offs))
    bs = None
    if term_groups is not None:
        bs, keep_b = bool_spec_of([(tg, 0) for tg in term_groups], len(offs))
    hp = None if has_pos is None else np.asarray(has_pos, np.uint8)
    nq = len(queries)
    qw, pw = np.zeros((max(nq, 1), 8), np.uint32), np.zeros((max(nq, 1), 8), np.uint32)
    vw, tw, bw = np.zeros((1024, 4), np.uint32), np.zeros((4096, 6), np.uint32), np.zeros((1024, 4), np.uint32)
    counts, err = (C.c_uint32 * 3)(), C.create_string_buffer(256)
    rc = L.slgp_plan_phrase(segs, None if hp is None else C.c_void_p(hp.ctypes.data), len(offs), nq,
                            None if bs is None else C.byref(bs), C.byref(sp), None, C.c_void_p(qw.ctypes.data),
                            C.c_void_p(pw.ctypes.data), C.c_void_p(vw.ctypes.data), 1024, C.c_void_p(tw.ctypes.data), 4096,
                            C.c_void_p(bw.ctypes.data), 1024, counts, err, 256)
    return rc, err.value.decode(), qw[:nq], pw[:nq], vw[:counts[0]], tw[:counts[1]], bw[:counts[2]]


def test_term_id_beyond_a_segments_dictionary():
    from searchlite_amd import _native as N
    offs = [[0, 3, 3, 10], [0, 5]]  # 3 terms, 1 term
    q = lambda t: [([(MUST, 0, [[t, (0, 0)]])], 0)]
    assert plan_phrase(q((2, 0)), offs)[0] == N.OK
    assert plan_phrase(q((2, N.NO_TERM)), offs)[0] == N.OK
    for bad in ((3, 0), (0, 1), (0xFFFFFFFE, 0)):
        rc, msg = plan_phrase(q(bad), offs)[:2]
        assert rc == N.ERR_INVALID and "term id out of range" in msg, (bad, rc, msg)


def test_tables_of_plan_phrase():
    """group numbering after the term groups, masks over both, min_should from the phrase spec; variants ordered
    MUST, MUST_NOT, SHOULD with the last-of-group flag; term rows in the spec's order with padded offsets (+ 64 per
    term) and unpadded bases; a variant with an absent or empty term, or in a segment without positions, has df 0
    in all its terms; a query without groups has nothing"""
    from searchlite_amd import _native as N
    offs = [[0, 3, 3, 10], [0, 5, 9]]  # segment 0: term 1 is empty; segment 1 has two terms
    NT = N.NO_TERM
    queries = [([(SHOULD, 2, [[(0, 0), (2, 1)], [(1, 1)]]), (MUST, 0, [[(2, NT), (0, 0)]]), (MUST_NOT, 7, [])], 2),
               ([], 7),
               ([(MUST_NOT, 1, [[(2, 1), (2, 1)]])], 0)]
    tgs = [[(MUST, [(0, 0)]), (SHOULD, [(2, 1)])], [], []]
    rc, msg, qw, pw, vw, tw, bw = plan_phrase(queries, offs, term_groups=tgs)
    assert rc == N.OK, msg
    # BoolQuery: term_begin, n_terms, must, must_not, should, min_should, n_must, n_must_not — phrase groups 2, 3, 4
    assert qw.tolist() == [[0, 2, 0b01001, 0b10000, 0b00110, 2, 1, 0], [2, 0, 0, 0, 0, 0, 0, 0], [2, 0, 0, 1, 0, 0, 0, 0]]
    # PhraseQuery: var_begin, n_vars, term_begin, n_terms, n_term_groups
    assert pw[:, :5].tolist() == [[0, 3, 0, 5, 2], [3, 0, 5, 0, 0], [3, 1, 5, 2, 0]]
    # PhraseVar: t_begin, n | last << 8, group, slop — the MUST phrase (group 3) first, then the SHOULD one's two
    assert vw.tolist() == [[3, 2 | 0x100, 3, 0], [0, 2, 2, 2], [2, 1 | 0x100, 2, 2], [0, 2 | 0x100, 0, 1]]
    rows = [(int(a) | (int(b) << 32), int(c) | (int(d) << 32), int(df)) for a, b, c, d, df, _ in tw]
    # query 0, segment 0: variant (0, 2) survives; variant (1) is empty there; variant (2, 0) survives
    assert rows[0:5] == [(0, 0, 3), (3 + 128, 3, 7), (3 + 64, 3, 0), (3 + 128, 3, 7), (0, 0, 3)]
    # query 0, segment 1: (0, 1) and (1) survive; (NO_TERM, 0) is dropped: df 0 in both terms
    assert rows[5:10] == [(0, 0, 5), (5 + 64, 5, 4), (5 + 64, 5, 4), (0, 0, 0), (0, 0, 0)]
    assert rows[10:] == [(3 + 128, 3, 7), (3 + 128, 3, 7), (5 + 64, 5, 4), (5 + 64, 5, 4)] and len(rows) == 14
    assert [(int(lo), int(df), int(g)) for lo, _, df, g in bw] == [(0, 3, 0), (3 + 128, 7, 1), (0, 5, 0), (5 + 64, 4, 1)]
    # a segment without positions: every variant is dropped there
    rc, msg, qw2, pw2, vw2, tw2, bw2 = plan_phrase(queries, offs, term_groups=tgs, has_pos=[1, 0])
    assert rc == N.OK and [int(r[4]) for r in tw2[5:10]] == [0] * 5 and [int(r[4]) for r in tw2[12:]] == [0, 0]
    assert tw2[:5].tolist() == tw[:5].tolist() and qw2.tolist() == qw.tolist() and vw2.tolist() == vw.tolist()


def check_positions(P_, offs, pos):
    L = plan_lib()
    L.slgp_check_positions.restype = C.c_int
    L.slgp_check_positions.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32]
    o = None if offs is None else np.asarray(offs, np.uint64)
    p = None if pos is None else np.asarray(pos, np.uint32)
    err = C.create_string_buffer(256)
    rc = L.slgp_check_positions(P_, None if o is None else o.ctypes.data, None if p is None else p.ctypes.data, err, 256)
    return rc, err.value.decode()


def test_set_positions_validation():
    from searchlite_amd import _native as N
    assert check_positions(3, [0, 2, 2, 5], [1, 1, 0, 4, 2 ** 31 - 1])[0] == N.OK  # equal positions, an empty posting
    assert check_positions(0, [0], None)[0] == N.OK
    for offs, pos, code, word in (
            (None, [1], N.ERR_INVALID, "pos_offsets is NULL"),
            ([1, 2, 3, 4], [0] * 4, N.ERR_INVALID, "start at 0"),
            ([0, 2, 1, 5], [0] * 5, N.ERR_INVALID, "not monotone"),
            ([0, 2, 2, 5], None, N.ERR_INVALID, "positions is NULL"),
            ([0, 2, 2, 5], [3, 2, 0, 1, 2], N.ERR_INVALID, "decrease inside posting 0"),
            ([0, 2, 2, 5], [3, 3, 5, 1, 2], N.ERR_INVALID, "decrease inside posting 2"),
            ([0, 2, 2, 5], [3, 3, 0, 1, 2 ** 31], N.ERR_INVALID, "2^31"),
            ([0, 2, 2, 2 ** 32], None, N.ERR_UNSUPPORTED, "2^32 - 1"),          # told from the offsets alone
            ([0, 2, 1, 2 ** 32], None, N.ERR_INVALID, "not monotone")):         # invalid before unsupported
        rc, msg = check_positions(3, offs, pos)
        assert rc == code and word in msg, (offs, pos, rc, msg)
