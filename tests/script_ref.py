"""Python restatement of script_score at the root of the score tree: CompiledScript::evaluate (query/script.rs:69-146)
and the ScriptScore node of evaluate_compiled_score (api/reader.rs:577-612), over programs in the form of
searchlite_amd.script.compile_script ([(op, arg)] in reverse Polish order), and over the oracle.

Per candidate doc with base score `base` (f32), on a stack of f64 (Python floats are IEEE f64, every operation below
is one correctly rounded operation):
  PUSH_CONST v       push v
  PUSH_FIELD id      push the doc's FIRST value of the column (an i64 value `as f64`), 0.0 when the doc has none
  PUSH_SCORE         push f64(base)
  ADD / SUB / MUL    pop b, pop a (an empty stack: NONE), val = a op b, not finite: NONE, push
  DIV                pop b, pop a, b == 0.0 (also -0.0): NONE, val = a / b, not finite: NONE, push
  NEG                pop a, val = -a, not finite: NONE, push
  a stack that does not hold exactly one value at the end: NONE; a value that is not finite: NONE; else f32(value).
The node: s = the script's value, NONE or not finite: NONE; score = s * f32(boost) in f32, not finite: NONE.  NONE
drops the doc: it is neither ranked nor counted.

evaluate() / node() are the scalar restatement, one doc at a time.  evaluate_docs() is the same over numpy arrays
(numpy's f64 add, subtract, multiply and divide are the same IEEE operations) for the device tests; the CPU tests
check it against the scalar form.

apply(): tests/fscore_ref.py's apply() over a CHAIN of stages per query, each ("script", entry) or ("fscore", spec) in
the order they run: a stage reads the score the stage before it left, and a doc dropped by any stage stays dropped
(evaluate_compiled_score evaluates a node's `base` with `?`)."""
import math

import numpy as np

from searchlite_amd import _native as N
from tests import fscore_ref

F32, F64 = np.float32, np.float64
PUSH_CONST, PUSH_FIELD, PUSH_SCORE = N.SCRIPT_PUSH_CONST, N.SCRIPT_PUSH_FIELD, N.SCRIPT_PUSH_SCORE
ADD, SUB, MUL, DIV, NEG = N.SCRIPT_ADD, N.SCRIPT_SUB, N.SCRIPT_MUL, N.SCRIPT_DIV, N.SCRIPT_NEG


def evaluate(program, field_value, base):
    """CompiledScript::evaluate for one doc.  field_value(id) -> the doc's first value of the column or None.
    -> numpy.float32, or None"""
    stack = []
    for op, arg in program:
        if op == PUSH_CONST:
            stack.append(float(arg))
        elif op == PUSH_FIELD:
            v = field_value(arg)
            stack.append(0.0 if v is None else float(v))
        elif op == PUSH_SCORE:
            stack.append(float(F32(base)))
        elif op == NEG:
            if not stack:
                return None
            val = -stack.pop()
            if not math.isfinite(val):
                return None
            stack.append(val)
        else:
            if len(stack) < 2:
                return None
            b = stack.pop()
            a = stack.pop()
            if op == DIV:
                if b == 0.0:
                    return None
                val = a / b
            else:
                # (Python raises no error for these; an overflow is inf)
                val = a + b if op == ADD else (a - b if op == SUB else a * b)
            if not math.isfinite(val):
                return None
            stack.append(val)
    if len(stack) != 1 or not math.isfinite(stack[0]):
        return None
    with np.errstate(over="ignore"):
        return F32(stack[0])


def node(program, boost, field_value, base):
    """the ScriptScore node for one doc -> numpy.float32, or None"""
    s = evaluate(program, field_value, base)
    if s is None or not np.isfinite(s):
        return None
    with np.errstate(over="ignore"):
        score = F32(s * F32(boost))
    return score if np.isfinite(score) else None


def well_formed(program):
    """no stack underflow and exactly one value at the end -> the deepest stack, or None"""
    depth = deepest = 0
    for op, _ in program:
        pops = 0 if op in (PUSH_CONST, PUSH_FIELD, PUSH_SCORE) else (1 if op == NEG else 2)
        if depth < pops:
            return None
        depth += 1 - pops
        deepest = max(deepest, depth)
    return deepest if depth == 1 else None


def evaluate_docs(entry, cols, s, docs, base):
    """one query's script_score over the docs of segment s with base scores `base` -> (score f32, kept).  entry:
    None (untouched), a program, or dict(program=, boost=); cols: fscore_ref.Columns"""
    base = np.asarray(base, F32)
    n = len(base)
    if entry is None:
        return base.copy(), np.ones(n, bool)
    if not isinstance(entry, dict):
        entry = dict(program=entry)
    program = entry["program"]
    if well_formed(program) is None:  # (also the empty program of `()`: its stack ends empty)
        return np.zeros(n, F32), np.zeros(n, bool)
    none = np.zeros(n, bool)
    stack = []
    with np.errstate(all="ignore"):
        for op, arg in program:
            if op == PUSH_CONST:
                stack.append(np.full(n, F64(arg)))
            elif op == PUSH_FIELD:
                val, has = cols.first(arg, s)
                stack.append(np.where(has[docs], val[docs], 0.0))
            elif op == PUSH_SCORE:
                stack.append(base.astype(F64))
            elif op == NEG:
                val = -stack.pop()
                none |= ~np.isfinite(val)
                stack.append(val)
            else:
                b = stack.pop()
                a = stack.pop()
                if op == DIV:
                    none |= b == 0.0
                    val = a / np.where(b == 0.0, 1.0, b)
                else:
                    val = a + b if op == ADD else (a - b if op == SUB else a * b)
                none |= ~np.isfinite(val)
                stack.append(val)
        value = stack[0]
        none |= ~np.isfinite(value)
        v = value.astype(F32)
        none |= ~np.isfinite(v)
        score = (v * F32(entry.get("boost", 1.0))).astype(F32)
        none |= ~np.isfinite(score)
    return score, ~none


def evaluate_stage(stage, cols, s, docs, base):
    kind, spec = stage
    if kind == "script":
        return evaluate_docs(spec, cols, s, docs, base)
    assert kind == "fscore", kind
    return fscore_ref.evaluate(spec, cols, s, docs, base)


def apply(cands, segs, chains, cols, k, q_filter=None):
    """fscore_ref.all_candidates() under one chain of stages per query -> (doc, seg, score, count) at k, scored_docs,
    matched, and per query the ranked survivors [(seg, doc, score)] (for a field sort on top)"""
    doc, seg, score, count = cands
    nq = len(count)
    out = (np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.uint32), np.zeros((nq, k), F32), np.zeros(nq, np.uint32))
    scored, matched, rows = np.zeros(nq, np.uint64), np.zeros(nq, np.uint64), []
    for q in range(nq):
        n = int(count[q])
        d, sg, sc = doc[q, :n].astype(np.int64), seg[q, :n].astype(np.int64), score[q, :n]
        new, kept, live = np.zeros(n, F32), np.zeros(n, bool), np.ones(n, bool)
        for s, sobj in enumerate(segs):
            at = np.nonzero(sg == s)[0]
            cur, keep = sc[at].astype(F32), np.ones(len(at), bool)
            for stage in chains[q]:
                cur, stage_keep = evaluate_stage(stage, cols, s, d[at], cur)
                keep &= stage_keep
            new[at], kept[at] = cur, keep
            if sobj.deleted is not None:
                live[at] &= ~np.unpackbits(np.asarray(sobj.deleted, np.uint8), bitorder="little")[d[at]].astype(bool)
            f = -1 if q_filter is None else int(q_filter[q])
            if f >= 0 and cols.filters[f][s] is not None:
                live[at] &= np.asarray(cols.filters[f][s], bool)[d[at]]
        scored[q] = int(kept.sum())
        at = np.nonzero(kept & live)[0]
        matched[q] = len(at)
        order = at[np.lexsort((d[at], sg[at], -fscore_ref.total_key(new[at])))]
        rows.append([(int(sg[i]), int(d[i]), new[i]) for i in order])
        m = min(k, len(order))
        out[0][q, :m], out[1][q, :m], out[2][q, :m], out[3][q] = d[order[:m]], sg[order[:m]], new[order[:m]], m
    return out, scored, matched, rows
