"""slg_batch_prepare_script / slg_search_batch_script argument checks that need no device: the spec is checked before
the index is looked at (a NULL index then fails with SLG_ERR_INVALID and a message, before anything touches a GPU);
field ids, the planned stack positions and the tables the kernel reads are checked through the host planner
(check_script / plan_script: pure host code); the header, the ctypes binding and the Rust mirror agree on the argument
counts and the spec's fields."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {"slg_batch_prepare_script": 13, "slg_search_batch_script": 19, "slg_batch_script_info": 3}

PC, PF, PS, ADD, SUB, MUL, DIV, NEG = range(8)  # SLG_SCRIPT_*
K = lambda v: (PC, v)
FLD = lambda f: (PF, f)
SCORE = (PS, 0)
OP = lambda op: (op, 0)
# `_score * 2 + f3` and `1 / f4`
TWO = [[SCORE, K(2.0), OP(MUL), FLD(3), OP(ADD)], dict(program=[K(1.0), FLD(4), OP(DIV)], boost=2.0)]


def left_nested(n_ops):
    """((1 + 1) + 1) + ...: 2 * n_ops + 1 instructions, depth 2"""
    return [K(1.0)] + [x for _ in range(n_ops) for x in (K(1.0), OP(ADD))]


def right_nested(depth):
    """1 + (1 + (1 + ...)): `depth` pushes, then depth - 1 operators"""
    return [K(1.0)] * depth + [OP(ADD)] * (depth - 1)


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


def spec_of(programs=None, **over):
    """the spec of one program per query (script.script_spec; default: TWO); over: fields replaced by an array (or
    n_consts by a number), or None for a NULL pointer -> (N.ScriptSpec, the arrays it points into)"""
    from searchlite_amd.script import script_spec
    programs = TWO if programs is None else programs
    sp, keep = script_spec(programs, len(programs))
    at = dict(p_offsets=0, i_op=1, i_arg=2, consts=3, q_boost=4)
    for name, v in over.items():
        if name == "n_consts":
            sp.n_consts = v
            continue
        i = at[name]
        if v is not None:
            keep[i] = np.ascontiguousarray(v, dtype=keep[i].dtype)
        setattr(sp, name, None if v is None else keep[i].ctypes.data)
    return sp, keep


def prepare(lib, spec, nq=2, k=11, order=0, fscore=None):
    offs = np.zeros(nq + 1, np.uint32)
    return lib.slg_batch_prepare_script(None, nq, offs.ctypes.data, None, None, None, None, None,
                                        None if spec is None else C.addressof(spec),
                                        None if fscore is None else C.addressof(fscore), order, k, 1)


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
    consts = ["SLG_MAX_SCRIPT_INSTRS", "SLG_MAX_SCRIPT_DEPTH", "SLG_MAX_SCRIPT_FIELDS", "SLG_SCRIPT_PUSH_CONST",
              "SLG_SCRIPT_PUSH_FIELD", "SLG_SCRIPT_PUSH_SCORE", "SLG_SCRIPT_ADD", "SLG_SCRIPT_SUB", "SLG_SCRIPT_MUL",
              "SLG_SCRIPT_DIV", "SLG_SCRIPT_NEG", "SLG_SCRIPT_OUTER", "SLG_SCRIPT_INNER"]
    fields = [n for n, _ in N.ScriptSpec._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(slg_script_spec));\n' +
                   "".join('  printf(" %%zu", offsetof(slg_script_spec, %s));\n' % f for f in fields) +
                   "".join('  printf(" %%d", (int)%s);\n' % c for c in consts) + '  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert out[0] == C.sizeof(N.ScriptSpec)
    assert out[1:1 + len(fields)] == [getattr(N.ScriptSpec, f).offset for f in fields]
    values = dict(zip(consts, out[1 + len(fields):]))
    assert (values["SLG_MAX_SCRIPT_INSTRS"], values["SLG_MAX_SCRIPT_DEPTH"], values["SLG_MAX_SCRIPT_FIELDS"]) == (64, 8, 8)
    assert [values[c] for c in consts[3:11]] == [PC, PF, PS, ADD, SUB, MUL, DIV, NEG]
    ffi = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    for name, val in values.items():
        assert getattr(N, name[4:]) == val, name
        assert re.search(r"pub const %s: \w+ = %d;" % (name, val), ffi), name
    body = re.search(r"pub struct slg_script_spec \{(.*?)\}", ffi, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", body) == fields
    assert lib.slg_abi_version() == 3


def test_null_spec_and_null_index(lib):
    rejected(lib, None, "ERR_INVALID", "script spec is NULL")
    rejected(lib, spec_of(), "ERR_INVALID", "index is NULL")  # a valid spec: the index is looked at next
    rejected(lib, spec_of(), "ERR_INVALID", "index is NULL", order=1)
    rejected(lib, spec_of([]), "ERR_INVALID", "index is NULL", nq=0)
    rejected(lib, spec_of([None, None]), "ERR_INVALID", "index is NULL")  # no query has a program


@pytest.mark.parametrize("name,word", [("p_offsets", "p_offsets"), ("q_boost", "q_boost"), ("i_op", "i_op/i_arg"),
                                       ("i_arg", "i_op/i_arg"), ("consts", "consts is NULL")])
def test_null_arrays(lib, name, word):
    rejected(lib, spec_of(**{name: None}), "ERR_INVALID", word)


def test_arrays_a_spec_does_not_need(lib):
    rejected(lib, spec_of([None, None], i_op=None, i_arg=None, consts=None), "ERR_INVALID", "index is NULL")
    rejected(lib, spec_of([[SCORE], [FLD(1), OP(NEG)]], consts=None), "ERR_INVALID", "index is NULL")  # no constant is pushed


def test_invalid_values(lib):
    rejected(lib, spec_of(p_offsets=np.array([0, 6, 5], np.uint32)), "ERR_INVALID", "p_offsets not monotone")
    rejected(lib, spec_of(i_op=[PS, PC, 8, PF, ADD, PC, PF, DIV]), "ERR_INVALID", "unknown script op")
    rejected(lib, spec_of(i_op=[PS, PC, MUL, PF, ADD, PC, PF, -1]), "ERR_INVALID", "unknown script op")
    rejected(lib, spec_of(i_arg=[0, 2, 0, 3, 0, 1, 4, 0]), "ERR_INVALID", "const index")
    rejected(lib, spec_of(i_arg=[0, -1, 0, 3, 0, 1, 4, 0]), "ERR_INVALID", "const index")
    rejected(lib, spec_of(n_consts=1), "ERR_INVALID", "const index")
    for bad in (np.inf, -np.inf, np.nan):
        rejected(lib, spec_of(q_boost=[1.0, bad]), "ERR_INVALID", "non-finite q_boost")
    rejected(lib, spec_of([None, None], q_boost=[np.nan, 1.0]), "ERR_INVALID", "non-finite q_boost")
    for order in (2, -1):
        rejected(lib, spec_of(), "ERR_INVALID", "unknown script order", order=order)


def test_limits(lib):
    # exactly at each limit: accepted (the index is looked at next)
    rejected(lib, spec_of([left_nested(31) + [OP(NEG)], None]), "ERR_INVALID", "index is NULL")   # 64 instructions
    rejected(lib, spec_of([None, right_nested(8)]), "ERR_INVALID", "index is NULL")                # depth 8
    eight = [FLD(0)] + [x for f in range(1, 8) for x in (FLD(f), OP(ADD))] + [FLD(0), OP(MUL)]
    rejected(lib, spec_of([eight, None]), "ERR_INVALID", "index is NULL")                          # 8 distinct fields
    # one over
    rejected(lib, spec_of([left_nested(32), None]), "ERR_UNSUPPORTED", "SLG_MAX_SCRIPT_INSTRS")    # 65
    rejected(lib, spec_of([None, right_nested(9)]), "ERR_UNSUPPORTED", "SLG_MAX_SCRIPT_DEPTH")
    nine = eight + [FLD(8), OP(ADD)]
    rejected(lib, spec_of([nine, None]), "ERR_UNSUPPORTED", "SLG_MAX_SCRIPT_FIELDS")


@pytest.mark.parametrize("program", [[K(1.0), K(2.0)], [OP(ADD)], [K(2.0), K(3.0)], [K(1.0), OP(ADD)], [OP(NEG)],
                                     [K(1.0), K(2.0), OP(ADD), OP(MUL)], [SCORE, K(1.0), OP(ADD), FLD(1)]])
def test_ill_formed_programs_are_unsupported(lib, program):
    """`1 2`, `+`, `2(3)`, ...: the reference compiles them and answers no hit; the device refuses them"""
    rejected(lib, spec_of([program, None]), "ERR_UNSUPPORTED", "ill-formed")


def test_non_finite_constants_are_unsupported(lib):
    for bad in (np.inf, -np.inf, np.nan):
        rejected(lib, spec_of([[SCORE, K(bad), OP(MUL)], None]), "ERR_UNSUPPORTED", "non-finite constant")
    # a constant no instruction pushes is not looked at
    rejected(lib, spec_of(consts=[2.0, 1.0, np.inf], n_consts=3), "ERR_INVALID", "index is NULL")


def test_an_invalid_argument_is_reported_before_an_unsupported_one(lib):
    rejected(lib, spec_of([right_nested(9), [K(1.0), OP(8)]]), "ERR_INVALID", "unknown script op")
    rejected(lib, spec_of([[K(1.0), K(2.0)], None], q_boost=[1.0, np.inf]), "ERR_INVALID", "non-finite q_boost")
    rejected(lib, spec_of([[OP(ADD)], None]), "ERR_INVALID", "unknown script order", order=7)


def test_the_fscore_spec_of_a_chain_is_checked_too(lib):
    from searchlite_amd.searcher import fscore_spec
    fs, keep = fscore_spec([dict(functions=[dict(kind="weight", weight=np.inf)]), None], 2)
    sp, keep2 = spec_of()
    assert prepare(lib, sp, fscore=fs) is None
    assert b"non-finite weight" in lib.slg_last_error()
    fs, keep = fscore_spec([dict(min_score=1.0), None], 2)
    for order in (0, 1):
        assert prepare(lib, sp, fscore=fs, order=order) is None
        assert b"index is NULL" in lib.slg_last_error()


def test_one_call_form_null_arguments(lib):
    from searchlite_amd import _native as N
    sp, keep = spec_of()
    args = (None, None, None, None, None, None)
    assert lib.slg_search_batch_script(None, 0, None, None, None, None, None, None, C.addressof(sp), None, 0, 11, 1, *args) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error()
    assert lib.slg_search_batch_script(None, 0, None, None, None, None, None, None, None, None, 0, 11, 1, *args) == N.ERR_INVALID
    assert b"script spec is NULL" in lib.slg_last_error()
    assert lib.slg_batch_script_info(None, None, None) == N.ERR_INVALID


# ---- the host planner: field ids against the registered fields, the stack positions and the tables ----
class Field(C.Structure):
    _fields_ = [("id", C.c_int32), ("keyword", C.c_uint32), ("non_finite", C.c_uint32), ("seg_has", C.c_void_p),
                ("seg_dense", C.c_void_p)]


INSTR = np.dtype([("code", "<u4"), ("pad", "<u4"), ("value", "<f8")])


def plan_script(programs, fields, n_segs=2, order=0):
    """fields: {id: dict(keyword=, non_finite=, has=[per segment], dense=[per segment])} -> (code, message, ScriptQuery
    words [nq, 16], ScriptInstr records, column addresses [n, 2], (n_work, max_depth)) of slgplan::plan_script"""
    from searchlite_amd import build
    L = C.CDLL(build.build_plan_lib())
    L.slgp_plan_script.restype = C.c_int
    keep, arr = [], (Field * max(len(fields), 1))()
    for i, (fid, f) in enumerate(fields.items()):
        has = np.array(f.get("has", [1] * n_segs), np.uint8)
        dense = np.array(f.get("dense", [0] * n_segs), np.uint8)
        keep += [has, dense]
        arr[i] = Field(fid, int(f.get("keyword", 0)), int(f.get("non_finite", 0)), has.ctypes.data, dense.ctypes.data)
    sp, keep2 = spec_of(programs)
    nq = len(programs)
    assert INSTR.itemsize == 16
    qw, ins = np.zeros((max(nq, 1), 16), np.uint32), np.zeros(1024, INSTR)
    cols = np.zeros((64, 2), np.uint64)
    counts, err = (C.c_uint32 * 4)(), C.create_string_buffer(256)
    rc = L.slgp_plan_script(arr, len(fields), n_segs, nq, C.byref(sp), order, C.c_void_p(qw.ctypes.data),
                            C.c_void_p(ins.ctypes.data), 1024, C.c_void_p(cols.ctypes.data), 64, counts, err, 256)
    return rc, err.value.decode(), qw[:nq], ins[:counts[0]], cols[:counts[1]], (counts[2], counts[3])


def test_ids_against_the_registered_fields():
    from searchlite_amd import _native as N
    fields = {3: {}, 4: dict(keyword=1), 5: dict(has=[1, 0]), 6: dict(non_finite=1)}
    one = lambda f: [[SCORE, FLD(f), OP(ADD)]]
    assert plan_script(one(3), fields)[0] == N.OK
    for f, code, word in ((7, N.ERR_INVALID, "unknown agg field id 7"), (-1, N.ERR_INVALID, "unknown agg field"),
                          (4, N.ERR_INVALID, "keyword"), (5, N.ERR_INVALID, "no column for segment 1"),
                          (6, N.ERR_UNSUPPORTED, "non-finite")):
        rc, msg = plan_script(one(f), fields)[:2]
        assert rc == code and word in msg, (f, rc, msg)
    # an invalid argument of a later query is reported before an unsupported column of an earlier one
    rc, msg = plan_script(one(6) + one(7), fields)[:2]
    assert rc == N.ERR_INVALID and "unknown agg field id 7" in msg
    assert plan_script(one(3), fields, order=2)[0] == N.ERR_INVALID


def test_limits_through_the_planner():
    from searchlite_amd import _native as N
    fields = {f: {} for f in range(9)}
    eight = [FLD(0)] + [x for f in range(1, 8) for x in (FLD(f), OP(ADD))] + [FLD(0), OP(MUL)]
    rc, msg, qw, ins, cols, (n_work, depth) = plan_script([left_nested(31) + [OP(NEG)], right_nested(8), eight], fields)
    assert rc == N.OK, msg
    assert qw[:, 1].tolist() == [64, 15, 17] and qw[:, 2].tolist() == [0, 0, 8] and qw[:, 4].tolist() == [2, 8, 2]
    assert (n_work, depth) == (3, 8) and len(cols) == 8 * 2
    for program, word in ((left_nested(32), "SLG_MAX_SCRIPT_INSTRS"), (right_nested(9), "SLG_MAX_SCRIPT_DEPTH"),
                          (eight + [FLD(8), OP(ADD)], "SLG_MAX_SCRIPT_FIELDS")):
        rc, msg = plan_script([program], fields)[:2]
        assert rc == N.ERR_UNSUPPORTED and word in msg, msg


def test_planned_stack_positions():
    """a left-nested program works at slots 0 and 1 only, a right-nested one climbs to slot 7 and comes back; a
    binary operator is planned at the slot of its LEFT operand, which is where its result goes"""
    from searchlite_amd import _native as N
    rc, msg, qw, ins, cols, (n_work, depth) = plan_script([left_nested(3), None, right_nested(8), [SCORE, OP(NEG)]], {})
    assert rc == N.OK, msg
    op, at = ins["code"] & 0xFF, (ins["code"] >> 8) & 0xFF
    assert qw[:, 0].tolist() == [0, 7, 7, 22] and qw[:, 1].tolist() == [7, 0, 15, 2]
    assert op[:7].tolist() == [PC, PC, ADD, PC, ADD, PC, ADD] and at[:7].tolist() == [0, 1, 0, 1, 0, 1, 0]
    assert at[7:22].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 6, 5, 4, 3, 2, 1, 0]
    assert op[22:].tolist() == [PS, NEG] and at[22:].tolist() == [0, 0]
    assert qw[:, 4].tolist() == [2, 0, 8, 1] and (n_work, depth) == (3, 8)


def test_tables_of_plan_script():
    from searchlite_amd import _native as N
    fields = {3: dict(dense=[1, 0]), 8: {}, 9: {}}
    # q0: f8 * f8 + f3 * 0.5 (f8 pushed twice: one field);  q2: (f3 - f9) / -2.5
    programs = [dict(program=[FLD(8), FLD(8), OP(MUL), FLD(3), K(0.5), OP(MUL), OP(ADD)], boost=-2.0), None,
                [FLD(3), FLD(9), OP(SUB), K(-2.5), OP(DIV)]]
    rc, msg, qw, ins, cols, (n_work, depth) = plan_script(programs, fields)
    assert rc == N.OK, msg
    f32 = lambda x: int(np.float32(x).view(np.uint32))
    # instr_begin, n_instrs, n_fields, boost, max_depth, pad x 3, col x 8 (rows of the column table, first use first)
    assert qw[0].tolist() == [0, 7, 2, f32(-2.0), 3, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert qw[1].tolist() == [7, 0, 0, f32(1.0), 0] + [0] * 11
    assert qw[2].tolist() == [7, 5, 2, f32(1.0), 2, 0, 0, 0, 1, 2, 0, 0, 0, 0, 0, 0]
    assert (n_work, depth) == (2, 3)
    code = lambda op, at, f=0: op | at << 8 | f << 16
    assert ins["code"].tolist() == [code(PF, 0, 0), code(PF, 1, 0), code(MUL, 0), code(PF, 1, 1), code(PC, 2), code(MUL, 1),
                                    code(ADD, 0), code(PF, 0, 0), code(PF, 1, 1), code(SUB, 0), code(PC, 1), code(DIV, 0)]
    assert ins["value"][4] == 0.5 and ins["value"][10] == -2.5 and not ins["pad"].any()
    addr = lambda owner, s, tag: ((owner + 1) << 32) | (s << 8) | tag
    # columns: field 8 first, then 3 (segment 0 stored without offsets), then 9
    assert cols.tolist() == [[addr(8, 0, 2), addr(8, 0, 1)], [addr(8, 1, 2), addr(8, 1, 1)],
                             [0, addr(3, 0, 1)], [addr(3, 1, 2), addr(3, 1, 1)],
                             [addr(9, 0, 2), addr(9, 0, 1)], [addr(9, 1, 2), addr(9, 1, 1)]]
