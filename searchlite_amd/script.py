"""script_score scripts for slg_batch_prepare_script: the reference's compiler (query/script.rs: tokenize,
read_number_literal, shunting_yard, compile_script) restated with its quirks, and the flat arrays of slg_script_spec.

The language: number literals (ASCII digits and at most one `.`), identifiers (`_score`, then a param, then a numeric
field), `+ - * /`, unary minus and parentheses.  Whitespace is space, tab, CR and LF only.  A `-` where an operand is
expected and that is directly followed by a digit or `.` starts a NEGATIVE LITERAL (`-0` is -0.0); any other `-` in
operand position is the unary operator Neg, which binds tighter than `* /` and is right-associative, so `-2 * 3` is
(-2) * 3 from a literal and `- 2 * 3` is Neg(2) * 3.  Errors raise ValueError with the reference's message.

A compiled program is a list of (op, arg) in reverse Polish order: (SCRIPT_PUSH_CONST, value), (SCRIPT_PUSH_FIELD, agg
field id), (SCRIPT_PUSH_SCORE, 0) and the operators with arg 0.  Params are constants by now.  The reference compiles
some scripts that can never give a hit (`1 2`, `+`, `2(3)`: the stack does not end with one value); so does this, and
the library answers such a program with SLG_ERR_UNSUPPORTED."""
from __future__ import annotations

import math

import numpy as np

from . import _native as N

MAX_SCRIPT_LENGTH = 512
MAX_SCRIPT_TOKENS = 128

# (precedence, right-associative)
_OPS = {N.SCRIPT_ADD: (1, False), N.SCRIPT_SUB: (1, False), N.SCRIPT_MUL: (2, False), N.SCRIPT_DIV: (2, False),
        N.SCRIPT_NEG: (3, True)}
_DIGITS = "0123456789"
_LETTERS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
# what Rust's str::trim removes (the Unicode White_Space property)
_RUST_WHITESPACE = "\t\n\x0b\x0c\r \x85\xa0\u1680" + "".join(chr(c) for c in range(0x2000, 0x200b)) + \
                   "\u2028\u2029\u202f\u205f\u3000"


def _read_number_literal(first: str, text: str, i: int):
    """read_number_literal: `first` is consumed, text[i:] follows -> (value, next index)"""
    num, dots, digits = "", 0, 0
    c = first
    while True:
        if c == ".":
            dots += 1
        elif c in _DIGITS:
            digits += 1
        num += c
        if dots > 1:
            raise ValueError(f"invalid number literal `{num}`")
        if i < len(text) and (text[i] in _DIGITS or text[i] == "."):
            c = text[i]
            i += 1
        else:
            break
    if digits == 0:
        raise ValueError(f"invalid number literal `{num}`")
    return float(num), i  # (Rust's f64 parse: `1.` and `.5` are numbers, too many digits give inf)


def tokenize(text: str) -> list:
    """-> tokens: ("num", value), ("ident", name), ("(",), (")",), ("op", SCRIPT_*)"""
    tokens, i, expect_operand = [], 0, True
    while i < len(text):
        ch = text[i]
        if ch in " \t\r\n":
            i += 1
        elif ch == "(":
            tokens.append(("(",))
            i += 1
            expect_operand = True
        elif ch == ")":
            tokens.append((")",))
            i += 1
            expect_operand = False
        elif ch == "-":
            i += 1
            if expect_operand:
                if i < len(text) and (text[i] in _DIGITS or text[i] == "."):
                    value, i = _read_number_literal(text[i], text, i + 1)
                    tokens.append(("num", -value))
                    expect_operand = False
                    continue
                tokens.append(("op", N.SCRIPT_NEG))
            else:
                tokens.append(("op", N.SCRIPT_SUB))
            expect_operand = True
        elif ch in "+*/":
            tokens.append(("op", {"+": N.SCRIPT_ADD, "*": N.SCRIPT_MUL, "/": N.SCRIPT_DIV}[ch]))
            i += 1
            expect_operand = True
        elif ch in _DIGITS or ch == ".":
            value, i = _read_number_literal(ch, text, i + 1)
            tokens.append(("num", value))
            expect_operand = False
        elif ch in _LETTERS or ch == "_":
            j = i
            while j < len(text) and (text[j] in _LETTERS or text[j] in _DIGITS or text[j] == "_"):
                j += 1
            tokens.append(("ident", text[i:j]))
            i = j
            expect_operand = False
        else:
            raise ValueError(f"unsupported character `{ch}` in script_score")
    return tokens


def shunting_yard(tokens: list) -> list:
    output, ops = [], []
    for tok in tokens:
        if tok[0] in ("num", "ident"):
            output.append(tok)
        elif tok[0] == "op":
            prec, right = _OPS[tok[1]]
            while ops and ops[-1][0] == "op":
                top = _OPS[ops[-1][1]][0]
                if top > prec or (top == prec and not right):
                    output.append(ops.pop())
                else:
                    break
            ops.append(tok)
        elif tok[0] == "(":
            ops.append(tok)
        else:
            found = False
            while ops:
                top = ops.pop()
                if top[0] == "(":
                    found = True
                    break
                if top[0] == "op":
                    output.append(top)
            if not found:
                raise ValueError("mismatched parentheses in script_score")
    while ops:
        top = ops.pop()
        if top[0] == "op":
            output.append(top)
        else:
            raise ValueError("mismatched parentheses in script_score")
    return output


def compile_script(text: str, params=None, field_ids=None) -> list:
    """The script as a program [(op, arg)].  params: {name: value} or None; field_ids: {name: agg field id} of the
    numeric fast fields a script may name.  An identifier is `_score`, else a param, else a field."""
    if not text.strip(_RUST_WHITESPACE):
        raise ValueError("script_score script cannot be empty")
    n_bytes = len(text.encode("utf-8"))
    if n_bytes > MAX_SCRIPT_LENGTH:
        raise ValueError(f"script_score script length {n_bytes} exceeds max {MAX_SCRIPT_LENGTH}")
    tokens = tokenize(text)
    if len(tokens) > MAX_SCRIPT_TOKENS:
        raise ValueError(f"script_score script is too large: {len(tokens)} tokens (max {MAX_SCRIPT_TOKENS})")
    rpn = shunting_yard(tokens)
    params = dict(params or {})
    for name in sorted(params):  # (a BTreeMap: in order of the names)
        if not math.isfinite(params[name]):
            raise ValueError(f"script_score param `{name}` must be finite")
    field_ids = field_ids or {}
    program = []
    for tok in rpn:
        if tok[0] == "num":
            program.append((N.SCRIPT_PUSH_CONST, tok[1]))
        elif tok[0] == "ident":
            name = tok[1]
            if name == "_score":
                program.append((N.SCRIPT_PUSH_SCORE, 0))
            elif name in params:
                program.append((N.SCRIPT_PUSH_CONST, float(params[name])))
            elif name in field_ids:
                program.append((N.SCRIPT_PUSH_FIELD, int(field_ids[name])))
            else:
                raise ValueError(f"script_score field `{name}` is not present in schema")
        elif tok[0] == "op":
            program.append((tok[1], 0))
    return program


def script_spec(programs, nq: int):
    """One script per query as (N.ScriptSpec, the arrays it points into).  programs[q]: None (the query is left as
    it is), a program of compile_script(), or a dict with `program` and `boost` (1.0: the script_score node's final
    boost).  A program without instructions (`()` compiles to one, and gives no hit in the reference) is refused
    with SLG_ERR_UNSUPPORTED: in the arrays, no instructions means "leave the query as it is"."""
    assert len(programs) == nq
    offs, ops, args, consts, boosts = [0], [], [], [], []
    for entry in programs:
        if entry is None:
            entry = dict(program=[])
        else:
            if not isinstance(entry, dict):
                entry = dict(program=entry)
            if not len(entry["program"]):
                raise N.SlgError(N.ERR_UNSUPPORTED, "a script without instructions gives no hit (CPU path)")
        for op, arg in entry["program"]:
            ops.append(int(op))
            if op == N.SCRIPT_PUSH_CONST:
                args.append(len(consts))
                consts.append(float(arg))
            else:
                args.append(int(arg))
        offs.append(len(ops))
        boosts.append(entry.get("boost", 1.0))
    pad = lambda a, dt: np.ascontiguousarray(a if len(a) else [0], dtype=dt)  # (never NULL: an empty array is read nowhere)
    keep = [pad(offs, np.uint32), pad(ops, np.int32), pad(args, np.int32), pad(consts, np.float64), pad(boosts, np.float32)]
    ptr = lambda a: a.ctypes.data
    return N.ScriptSpec(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), len(consts), ptr(keep[4])), keep
