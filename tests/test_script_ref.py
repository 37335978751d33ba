"""tests/script_ref.py and searchlite_amd/script.py against hand-derived cases of the reference's script language
(query/script.rs) and its ScriptScore node (api/reader.rs:577-612).  No device."""
import math

import numpy as np
import pytest

from searchlite_amd import _native as N
from searchlite_amd.script import compile_script, script_spec
from tests import fscore_ref
from tests import script_ref as R

F32 = np.float32
C, F, S = N.SCRIPT_PUSH_CONST, N.SCRIPT_PUSH_FIELD, N.SCRIPT_PUSH_SCORE
ADD, SUB, MUL, DIV, NEG = (N.SCRIPT_ADD, 0), (N.SCRIPT_SUB, 0), (N.SCRIPT_MUL, 0), (N.SCRIPT_DIV, 0), (N.SCRIPT_NEG, 0)
FIELDS = {"popularity": 3, "x": 4, "a": 5}


def run(text, base=1.0, boost=1.0, params=None, values=None):
    """the node's score of one doc whose fields have `values` ({name: value}; a missing name: no value)"""
    values = values or {}
    by_id = {FIELDS[n]: v for n, v in values.items()}
    return R.node(compile_script(text, params, FIELDS), boost, by_id.get, base)


def test_the_references_own_case():
    """tests/function_score.rs:361: `_score + popularity * 0.1` ranks popularity 10 > 5 > 1 on equal base scores"""
    assert compile_script("_score + popularity * 0.1", None, FIELDS) == [(S, 0), (F, 3), (C, 0.1), MUL, ADD]
    got = [run("_score + popularity * 0.1", 1.0, values=dict(popularity=p)) for p in (10, 1, 5)]
    assert got == [F32(1.0 + 10 * 0.1), F32(1.0 + 1 * 0.1), F32(1.0 + 5 * 0.1)]
    assert got[0] > got[2] > got[1]
    assert got[0].dtype == np.float32


def test_precedence_and_associativity():
    assert compile_script("2 - 3 - 4") == [(C, 2.0), (C, 3.0), SUB, (C, 4.0), SUB]  # left-associative
    assert run("2 - 3 - 4") == F32(-5.0)
    assert run("2 * 3 + 4 * 5") == F32(26.0) and run("2 * (3 + 4) * 5") == F32(70.0)
    assert run("8 / 4 / 2") == F32(1.0) and run("8 / (4 / 2)") == F32(4.0)
    # unary minus binds tighter than * and is right-associative
    assert compile_script("2 * -x", None, FIELDS) == [(C, 2.0), (F, 4), NEG, MUL]
    assert run("2 * -x", values=dict(x=3.0)) == F32(-6.0)
    assert compile_script("- -x", None, FIELDS) == [(F, 4), NEG, NEG]
    assert run("- -x", values=dict(x=3.0)) == F32(3.0)
    # a `-` in operand position directly in front of a digit is a negative literal, otherwise Neg
    assert compile_script("2 - -3") == [(C, 2.0), (C, -3.0), SUB] and run("2 - -3") == F32(5.0)
    assert compile_script("-2 * 3") == [(C, -2.0), (C, 3.0), MUL]
    assert compile_script("- 2 * 3") == [(C, 2.0), NEG, (C, 3.0), MUL]
    assert run("-2 * 3") == run("- 2 * 3") == F32(-6.0)
    assert compile_script("-.5") == [(C, -0.5)] and compile_script("1.") == [(C, 1.0)]
    assert compile_script("2-3") == [(C, 2.0), (C, 3.0), SUB]  # after an operand `-` is Sub, whatever follows
    assert compile_script("(2)-3") == [(C, 2.0), (C, 3.0), SUB]
    assert compile_script("2 - - 3") == [(C, 2.0), (C, 3.0), NEG, SUB]
    # Neg sits above a lower operator on the stack until that operand is complete
    assert compile_script("-x + 1", None, FIELDS) == [(F, 4), NEG, (C, 1.0), ADD]
    (op, v), = compile_script("-0")
    assert op == C and v == 0.0 and math.copysign(1.0, v) == -1.0  # -0.0
    assert compile_script(" \t\r\n1\n") == [(C, 1.0)]


def test_division():
    assert run("a / 0", values=dict(a=3.0)) is None
    assert run("a / -0", values=dict(a=3.0)) is None  # -0.0 == 0.0
    assert run("a / (1 - 1)", values=dict(a=3.0)) is None
    assert run("0 / a", values=dict(a=3.0)) == F32(0.0)
    assert run("0 / a", values={}) is None  # a missing value is 0.0, so this is 0 / 0
    assert run("1 / 3") == F32(1.0 / 3.0)
    tiny = 5e-324
    assert run("a / t", params=dict(t=tiny), values=dict(a=1.0)) is None  # the quotient is inf


def test_overflows():
    big = 1e200
    assert run("b * b", params=dict(b=big)) is None                      # the product is inf in f64
    assert run("b + b", params=dict(b=1.7e308)) is None and run("0 - b - b", params=dict(b=1.7e308)) is None
    assert run("b", params=dict(b=1e39)) is None                          # finite in f64, inf as f32
    assert run("b", params=dict(b=3e38)) == F32(3e38)
    assert run("b", params=dict(b=3e38), boost=2.0) is None               # v * boost overflows
    assert run("b", params=dict(b=3e38), boost=-2.0) is None
    assert run("b * 0", params=dict(b=1e200)) == F32(0.0)
    # the f64 value rounds to f32 only at the end
    assert run("b + 1 - b", params=dict(b=2.0 ** 60)) == F32(0.0)
    assert run("_score + 1", base=F32(2.0 ** 24)) == F32(2.0 ** 24 + 1.0)  # exact in f64, rounded to even as f32


def test_boost_and_base():
    assert run("_score * 2", base=1.5, boost=-1.0) == F32(-3.0)
    assert run("_score", base=F32(0.1), boost=1.0) == F32(0.1)           # f32 -> f64 -> f32 is the identity
    assert run("_score", base=F32(0.1), boost=0.0) == F32(0.0)
    assert run("_score", base=F32(np.inf)) is None and run("1 / _score", base=F32(np.inf)) == F32(0.0)
    got = run("0 - _score", base=0.0, boost=1.0)
    assert got == 0.0
    got = run("-_score", base=0.0)
    assert got == 0.0 and np.signbit(got)                                 # Neg of +0.0 is -0.0


def test_fields_and_params():
    assert run("x + 1", values={}) == F32(1.0)                            # a missing value is 0.0
    assert run("x + 1", values=dict(x=None)) == F32(1.0)
    assert run("x + 1", values=dict(x=2 ** 53 + 1)) == F32(float(2 ** 53 + 1) + 1.0)  # an i64 value `as f64`
    # a param shadows a field of the same name; `_score` shadows both
    assert compile_script("x", dict(x=7.0), FIELDS) == [(C, 7.0)]
    assert run("x", params=dict(x=7.0), values=dict(x=1.0)) == F32(7.0)
    assert compile_script("_score", dict(_score=7.0), {"_score": 9}) == [(S, 0)]
    assert compile_script("x * x + x", None, FIELDS) == [(F, 4), (F, 4), MUL, (F, 4), ADD]
    assert compile_script("a1_b", None, {"a1_b": 2}) == [(F, 2)]


@pytest.mark.parametrize("text,params,message", [
    ("", None, "script_score script cannot be empty"),
    (" \t\n", None, "script_score script cannot be empty"),
    ("\u2003\n", None, "script_score script cannot be empty"),              # (str::trim: Unicode whitespace)
    ("1 +" + " " * 510, None, "script_score script length 513 exceeds max 512"),
    ("é" * 257, None, "script_score script length 514 exceeds max 512"),    # bytes, not characters
    ("+".join(["1"] * 65), None, "script_score script is too large: 129 tokens (max 128)"),
    ("1..2", None, "invalid number literal `1..`"),
    ("1.2.3", None, "invalid number literal `1.2.`"),
    (".", None, "invalid number literal `.`"),
    ("-.", None, "invalid number literal `.`"),
    ("..", None, "invalid number literal `..`"),
    ("1 % 2", None, "unsupported character `%` in script_score"),
    ("1 \u00a0+ 2", None, "unsupported character `\u00a0` in script_score"),  # not one of the four whitespace characters
    ("1e5", None, "script_score field `e5` is not present in schema"),      # no exponents: `1` then an identifier
    ("x ^ 2", None, "unsupported character `^` in script_score"),
    ("é", None, "unsupported character `é` in script_score"),
    ("(1 + 2", None, "mismatched parentheses in script_score"),
    ("1 + 2)", None, "mismatched parentheses in script_score"),
    (")(", None, "mismatched parentheses in script_score"),
    ("nope + 1", None, "script_score field `nope` is not present in schema"),
    ("p", dict(p=math.inf), "script_score param `p` must be finite"),
    ("1", dict(b=math.nan, a=math.inf), "script_score param `a` must be finite"),  # in order of the names, used or not
    ("nope", dict(p=math.nan), "script_score param `p` must be finite"),    # params are checked before identifiers
    ("(1", dict(p=math.nan), "mismatched parentheses in script_score"),     # ... and after the parse
])
def test_compile_errors(text, params, message):
    with pytest.raises(ValueError) as ei:
        compile_script(text, params, FIELDS)
    assert str(ei.value) == message


def test_limits_that_are_not_errors():
    assert len(compile_script("1 +" + " " * 509)) == 2                      # 512 bytes (ill-formed, compiled)
    assert len(compile_script("+".join(["1"] * 64) + "+")) == 128           # 128 tokens (ill-formed, compiled)
    assert compile_script("1" * 400) == [(C, math.inf)]                    # too many digits: inf, compiled


@pytest.mark.parametrize("text", ["1 2", "+", "2(3)", "1 +", "()", "* 2", "-", "1 2 +  3"])
def test_ill_formed_programs_compile_and_give_none(text):
    program = compile_script(text)
    assert R.well_formed(program) is None
    assert R.node(program, 1.0, lambda f: None, 1.0) is None
    cols = fscore_ref.Columns([])
    score, kept = R.evaluate_docs(program, cols, 0, np.arange(3), np.ones(3, F32))
    assert not kept.any()


def test_a_non_finite_literal_gives_none():
    assert R.node(compile_script("1" * 400), 1.0, lambda f: None, 1.0) is None
    assert R.node(compile_script("_score + 0 * " + "1" * 400), 1.0, lambda f: None, 1.0) is None  # 0 * inf


def test_well_formed_depth():
    assert R.well_formed(compile_script("1 + (2 + (3 + (4 + (5 + (6 + (7 + 8))))))")) == 8
    assert R.well_formed(compile_script("1 + 2 + 3 + 4 + 5")) == 2
    assert R.well_formed([]) is None


def test_vector_form_equals_the_scalar_form():
    """evaluate_docs (numpy, what the device tests use) against node() doc by doc, NONE cases included"""
    rng = np.random.default_rng(5)

    class Seg:
        n_docs, deleted = 400, None

    vals = [[[float(rng.choice([0.0, -0.0, 1.0, -2.5, 1e200, 1e-200, 3e38, 7.0]))] if rng.random() < 0.8 else []
             for _ in range(400)]]
    ints = [[[int(rng.integers(-5, 6))] for _ in range(400)]]
    cols = fscore_ref.Columns([Seg], {4: (vals, np.dtype(np.float64)), 5: (ints, np.dtype(np.int64))})
    docs = np.arange(400)
    base = rng.uniform(-2, 2, 400).astype(F32)
    base[::7] = 0.0
    texts = ["_score", "x * x", "x / a", "a / x", "_score / (x - 1)", "-x * big", "x + 1 - x", "1 / (a * _score)",
             "x * ten", "(x + a) * (x - a) / (_score + 1)", "- - a / - x"]
    checked = dropped = 0
    for text in texts:
        for boost in (1.0, -2.5, 1e30):
            program = compile_script(text, dict(big=1e200, ten=1e10), FIELDS)
            score, kept = R.evaluate_docs(dict(program=program, boost=boost), cols, 0, docs, base)
            for d in docs:
                fv = lambda f: (vals if f == 4 else ints)[0][d][0] if (vals if f == 4 else ints)[0][d] else None
                want = R.node(program, boost, fv, base[d])
                assert kept[d] == (want is not None), (text, boost, d)
                if want is not None:
                    assert score[d].view(np.uint32) == want.view(np.uint32), (text, boost, d)
                    checked += 1
                else:
                    dropped += 1
    assert checked > 3000 and dropped > 1000
    # untouched entries
    score, kept = R.evaluate_docs(None, cols, 0, docs, base)  # an untouched query
    assert kept.all() and np.array_equal(score.view(np.uint32), base.view(np.uint32))


def test_script_spec_arrays():
    programs = [compile_script("_score * w + x", dict(w=0.5), FIELDS), None,
                dict(program=compile_script("2 / a", None, FIELDS), boost=-1.5), None]
    spec, keep = script_spec(programs, 4)
    offs, ops, args, consts, boost = keep
    assert offs.tolist() == [0, 5, 5, 8, 8] and offs.dtype == np.uint32
    assert ops.tolist() == [S, C, N.SCRIPT_MUL, F, N.SCRIPT_ADD, C, F, N.SCRIPT_DIV] and ops.dtype == np.int32
    assert args.tolist() == [0, 0, 0, 4, 0, 1, 5, 0] and args.dtype == np.int32
    assert consts.tolist() == [0.5, 2.0] and consts.dtype == np.float64 and spec.n_consts == 2
    assert boost.tolist() == [1.0, 1.0, -1.5, 1.0] and boost.dtype == np.float32
    assert spec.p_offsets == offs.ctypes.data and spec.q_boost == boost.ctypes.data
    spec, keep = script_spec([], 0)
    assert spec.n_consts == 0 and spec.p_offsets
    # `()` compiles to a program without instructions, which gives no hit; in the arrays no instructions means
    # "leave the query as it is", so it is refused here
    for empty in ([], dict(program=compile_script("()"))):
        with pytest.raises(N.SlgError) as ei:
            script_spec([empty], 1)
        assert ei.value.code == N.ERR_UNSUPPORTED
