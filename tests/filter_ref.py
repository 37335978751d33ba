"""The non-nested part of the reference's filter evaluation (searchlite-core/src/query/filters.rs:84-149 over
index/fastfields.rs:475-640), restated doc by doc in plain Python over per-doc value lists: the CPU side of
tests/test_gpu_filter_trees.py and what tests/test_filter_ref.py checks against hand-derived cases.

A field is dict(kind="keyword" | "i64" | "f64", keys=[dictionary strings] (keyword), id=agg field id,
docs=[per segment: a list of n_docs lists of values (keyword: ordinals into keys), or None = the segment has no
value at all]).  Nothing here shares code with searchlite_amd.filters: strings are compared here, ordinals there.
"""
import numpy as np


def case_insensitive_equals(a: str, b: str) -> bool:
    """fastfields.rs:475-481"""
    if a.isascii() and b.isascii():
        return a.casefold() == b.casefold()  # eq_ignore_ascii_case (casefold of an ASCII string is its ASCII fold)
    return a.lower() == b.lower()            # to_lowercase on both


def _any(field, seg, n_docs, pred):
    """matches_*: ANY value of the doc satisfies pred; a doc without a value, or a segment without the column: no"""
    docs = field["docs"][seg]
    if docs is None:
        return np.zeros(n_docs, dtype=bool)
    assert len(docs) == n_docs
    return np.array([any(pred(v) for v in vals) for vals in docs], dtype=bool).reshape(n_docs)


def eval_filter(flt, fields, seg, n_docs, nested=None):
    """filter_matches (filters.rs:84-149) for every doc of one segment -> bool[n_docs].  A field that does not
    exist or is of another kind matches nothing (fastfields.rs `_ => false`).  nested(path, filter, seg) -> the
    mask of a Nested node (evaluated elsewhere); And hands the Nested children of one path over together
    (passes_filters_at, filters.rs:13-50)."""
    (tag, body), = flt.items()
    never = np.zeros(n_docs, dtype=bool)
    if tag in ("KeywordEq", "KeywordIn"):
        f = fields.get(body["field"])
        if f is None or f["kind"] != "keyword":
            return never
        wanted = [body["value"]] if tag == "KeywordEq" else list(body["values"])
        return _any(f, seg, n_docs, lambda o: any(case_insensitive_equals(f["keys"][o], w) for w in wanted))
    if tag == "I64Range":
        f = fields.get(body["field"])
        if f is None or f["kind"] != "i64":
            return never
        lo, hi = int(body["min"]), int(body["max"])
        return _any(f, seg, n_docs, lambda v: int(v) >= lo and int(v) <= hi)
    if tag == "F64Range":
        f = fields.get(body["field"])
        if f is None or f["kind"] != "f64":
            return never
        lo, hi = float(body["min"]), float(body["max"])
        return _any(f, seg, n_docs, lambda v: float(v) >= lo and float(v) <= hi)
    if tag == "Nested":
        return np.asarray(nested(body["path"], body["filter"], seg), dtype=bool)
    if tag == "And":
        out = np.ones(n_docs, dtype=bool)  # (an empty list passes)
        groups = {}
        for child in body:
            if list(child) == ["Nested"]:
                groups.setdefault(child["Nested"]["path"], []).append(child["Nested"]["filter"])
            else:
                out &= eval_filter(child, fields, seg, n_docs, nested)
        for path, group in groups.items():
            out &= np.asarray(nested(path, group[0] if len(group) == 1 else {"And": group}, seg), dtype=bool)
        return out
    if tag == "Or":
        out = never.copy()  # (`any` over nothing is false)
        for child in body:
            out |= eval_filter(child, fields, seg, n_docs, nested)
        return out
    if tag == "Not":
        return ~eval_filter(body, fields, seg, n_docs, nested)
    raise ValueError(tag)


def eval_program(nodes, ords, fields_by_id, filter_pass, seg, n_docs):
    """A postfix program as slg_index_add_filter_trees takes it (nodes: dicts of slg_filter_node fields), doc by
    doc -> bool[n_docs].  filter_pass: filter id -> per segment the mask a FILTER_ID leaf reads (the filter's pass
    bits: alive and passing).  I64 bounds are compared as integers, as the reference does."""
    stack = []
    for nd in nodes:
        kind = nd["kind"]
        if kind == 0:
            f = fields_by_id[nd["field"]]
            b = nd.get("ord_begin", 0)
            wanted = set(int(o) for o in ords[b:b + nd.get("n_ords_in", 0)])
            stack.append(_any(f, seg, n_docs, lambda o: int(o) in wanted))
        elif kind == 1:
            lo, hi = nd["lo_f"], nd["hi_f"]
            stack.append(_any(fields_by_id[nd["field"]], seg, n_docs, lambda v: lo <= float(v) and float(v) <= hi))
        elif kind == 2:
            lo, hi = nd["lo_i"], nd["hi_i"]
            stack.append(_any(fields_by_id[nd["field"]], seg, n_docs, lambda v: lo <= int(v) and int(v) <= hi))
        elif kind == 3:
            stack.append(np.asarray(filter_pass[nd["filter_id"]][seg], dtype=bool).copy())
        elif kind == 6:
            stack.append(~stack.pop())
        else:
            n = nd.get("arity", 0)
            kids = [stack.pop() for _ in range(n)]
            out = np.ones(n_docs, dtype=bool) if kind == 4 else np.zeros(n_docs, dtype=bool)
            for kmask in kids:
                out = (out & kmask) if kind == 4 else (out | kmask)
            stack.append(out)
    assert len(stack) == 1
    return stack[0]
