"""Filter trees for the device (slg_index_add_filter_trees): request -> postfix program.

The reference's `filter` (api/types.rs: KeywordEq, KeywordIn, I64Range, F64Range, Nested, And, Or, Not, in serde's
externally tagged JSON form, e.g. {"And": [{"KeywordEq": {"field": "cat", "value": "news"}}, ...]}) is evaluated per
doc by query/filters.rs over the fast fields.  The device evaluates the same tree over the columns registered with
GpuIndex.add_agg_field / add_agg_keyword_field; what is host work lives here: walking the JSON into postfix order
and resolving keyword strings to the ordinals of the column's dictionary with the reference's
case_insensitive_equals (index/fastfields.rs:475-481), under which several dictionary keys may equal one value.

A leaf the reference answers `false` for every doc (a field that does not exist, or one of another kind:
fastfields.rs `_ => false`; an F64Range with a NaN bound) compiles to OR of nothing, which is false.

Nested nodes: compile_filter hands them to a callback (a host-made bitmap named by FILTER_ID); compile_nested_filter
compiles them for the device (slg_index_add_nested_filter_trees: one object scope per Nested node or group, over the
nested paths and columns registered with GpuIndex.add_nested_path / add_nested_field / add_nested_keyword_field),
and nested_columns maps a segment's nested fast-field columns onto those registrations.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from . import _native as N


def case_insensitive_equals(a: str, b: str) -> bool:
    """index/fastfields.rs:475-481: ASCII case fold when both sides are ASCII, else to_lowercase on both."""
    # (one expression serves both: on ASCII strings str.lower is the ASCII fold, elsewhere it is Unicode's full
    # lowercasing, as Rust's to_lowercase)
    return a.lower() == b.lower()


class FilterProgram:
    """One tree as slg_filter_tree takes it: .nodes, dicts of slg_filter_node fields in postfix order, and .ords,
    the ordinals its KEYWORD_IN nodes point into."""

    def __init__(self, nodes: List[dict], ords: List[int]):
        self.nodes = nodes
        self.ords = ords


def compile_filter(filter_json: dict, fields: Dict[str, dict],
                   nested: Optional[Callable[[str, dict], int]] = None) -> FilterProgram:
    """filter_json: the reference's filter; fields: field name -> {"id": agg field id, "kind": "keyword" | "i64"
    | "f64", "keys": [dictionary strings] (keyword fields)}; nested(path, filter) -> the id of a registered filter
    that stands for a Nested node (the caller evaluates that sub-tree and registers its bitmap; the Nested children
    of one And that share a path arrive as one call with their And).  Without the
    callback a Nested node raises SlgError(ERR_UNSUPPORTED); a malformed filter raises ValueError."""
    nodes: List[dict] = []
    ords: List[int] = []

    def never():
        nodes.append(dict(kind=N.FILTER_OR, arity=0))

    def keyword(field: str, values: Sequence[str]):
        f = fields.get(field)
        if f is None or f.get("kind") != "keyword":
            return never()
        begin = len(ords)
        ords.extend(o for o, key in enumerate(f["keys"]) if any(case_insensitive_equals(key, v) for v in values))
        nodes.append(dict(kind=N.FILTER_KEYWORD_IN, field=int(f["id"]), ord_begin=begin, n_ords_in=len(ords) - begin))

    def nested_leaf(path: str, flt: dict):
        if nested is None:
            raise N.SlgError(N.ERR_UNSUPPORTED, "a Nested filter is not evaluated on the device: pass nested= to "
                                                "register its bitmap and name it by id")
        nodes.append(dict(kind=N.FILTER_ID, filter_id=int(nested(path, flt))))

    def walk(flt):
        if not isinstance(flt, dict) or len(flt) != 1:
            raise ValueError(f"a filter is an object with one key, got {flt!r}")
        (tag, body), = flt.items()
        if tag == "KeywordEq":
            keyword(body["field"], [body["value"]])
        elif tag == "KeywordIn":
            keyword(body["field"], list(body["values"]))
        elif tag == "I64Range":
            f = fields.get(body["field"])
            if f is None or f.get("kind") != "i64":
                return never()
            nodes.append(dict(kind=N.FILTER_RANGE_I64, field=int(f["id"]), lo_i=int(body["min"]), hi_i=int(body["max"])))
        elif tag == "F64Range":
            f = fields.get(body["field"])
            lo, hi = float(body["min"]), float(body["max"])
            if f is None or f.get("kind") != "f64" or math.isnan(lo) or math.isnan(hi):
                return never()
            nodes.append(dict(kind=N.FILTER_RANGE_F64, field=int(f["id"]), lo_f=lo, hi_f=hi))
        elif tag == "Nested":
            nested_leaf(body["path"], body["filter"])
        elif tag == "And":
            # passes_filters_at (filters.rs:13-50): the Nested children of one path must hold for ONE object of that
            # path, so they reach the callback together, as one And
            groups: Dict[str, list] = {}
            plain = 0
            for child in body:
                if isinstance(child, dict) and list(child) == ["Nested"]:
                    groups.setdefault(child["Nested"]["path"], []).append(child["Nested"]["filter"])
                else:
                    walk(child)
                    plain += 1
            for path, group in groups.items():
                nested_leaf(path, group[0] if len(group) == 1 else {"And": group})
            nodes.append(dict(kind=N.FILTER_AND, arity=plain + len(groups)))
        elif tag == "Or":
            for child in body:
                walk(child)
            nodes.append(dict(kind=N.FILTER_OR, arity=len(body)))
        elif tag == "Not":
            walk(body)
            nodes.append(dict(kind=N.FILTER_NOT))
        else:
            raise ValueError(f"unknown filter {tag!r}")

    walk(filter_json)
    return FilterProgram(nodes, ords)


def tree_array(trees):
    """trees: FilterProgram objects or (nodes, ords) pairs -> (an N.FilterTree array of len(trees) entries (one
    unused entry when there is none), what it points into)."""
    arr = (N.FilterTree * max(len(trees), 1))()
    keep = []
    names = [n for n, _ in N.FilterNode._fields_]
    for t, tree in enumerate(trees):
        nodes, ords = (tree.nodes, tree.ords) if isinstance(tree, FilterProgram) else tree
        na = (N.FilterNode * max(len(nodes), 1))()
        for i, nd in enumerate(nodes):
            unknown = set(nd) - set(names)
            if unknown:
                raise KeyError(f"slg_filter_node has no field {sorted(unknown)}")
            for name, v in nd.items():
                setattr(na[i], name, v)
        oa = np.ascontiguousarray(ords, dtype=np.uint32)
        keep += [na, oa]
        arr[t] = N.FilterTree(len(nodes), C.addressof(na), len(oa), oa.ctypes.data if len(oa) else None)
    return arr, keep


# ---- nested filters (slg_index_add_nested_filter_trees) -----------------------------------------------------------
class NestedFilterProgram:
    """One tree as slg_nested_filter_tree takes it: .scopes, (path id, node_begin, n_nodes) rows with children before
    parents and the doc level (path -1) last; .nodes, every scope's postfix program back to back; .ords."""

    def __init__(self, scopes: List[tuple], nodes: List[dict], ords: List[int]):
        self.scopes = scopes
        self.nodes = nodes
        self.ords = ords


def compile_nested_filter(filter_json: dict, fields: Dict[str, dict], nested: dict) -> NestedFilterProgram:
    """filter_json, fields: as compile_filter's (the doc-level columns).  nested: {"paths": {full path: {"id": nested
    path id}}, "fields": {"<full path>.<field>": {"id": nested field id, "path": full path, "kind": "keyword" | "i64"
    | "f64", "keys": [dictionary strings] (keyword fields)}}}.

    Restates query/filters.rs:13-188.  A Nested node opens an object scope at base.path; inside it a leaf reads the
    nested column `full path.field` (a doc-level column named there matches nothing); the Nested children of ONE And
    that share a path become ONE scope whose program ANDs them (passes_filters_at), at every level; under Or and
    Not, and alone, each Nested node has a scope of its own.  An unknown path or field, or one of another kind,
    compiles to OR of nothing, which is false."""
    paths, nfields = nested.get("paths", {}), nested.get("fields", {})
    scopes: List[tuple] = []  # (path id, nodes), children before parents
    ords: List[int] = []

    def leaf(out, base, field, kind, make):
        if base:
            f = nfields.get(f"{base}.{field}")
            if f is not None and f.get("path") != base:
                f = None
        else:
            f = fields.get(field)
        if f is None or f.get("kind") != kind:
            out.append(dict(kind=N.FILTER_OR, arity=0))
        else:
            out.append(make(f))

    def keyword(f, values):
        begin = len(ords)
        ords.extend(o for o, key in enumerate(f["keys"]) if any(case_insensitive_equals(key, v) for v in values))
        return dict(kind=N.FILTER_KEYWORD_IN, field=int(f["id"]), ord_begin=begin, n_ords_in=len(ords) - begin)

    def nested_leaf(out, base, path, flt):
        full = f"{base}.{path}" if base else path
        if full not in paths:  # nested_object_count is 0 for every doc
            out.append(dict(kind=N.FILTER_OR, arity=0))
            return
        inner: List[dict] = []
        walk(inner, full, flt)
        scopes.append((int(paths[full]["id"]), inner))
        out.append(dict(kind=N.FILTER_NESTED, field=len(scopes) - 1))

    def walk(out, base, flt):
        if not isinstance(flt, dict) or len(flt) != 1:
            raise ValueError(f"a filter is an object with one key, got {flt!r}")
        (tag, body), = flt.items()
        if tag == "KeywordEq":
            leaf(out, base, body["field"], "keyword", lambda f: keyword(f, [body["value"]]))
        elif tag == "KeywordIn":
            leaf(out, base, body["field"], "keyword", lambda f: keyword(f, list(body["values"])))
        elif tag == "I64Range":
            leaf(out, base, body["field"], "i64", lambda f: dict(kind=N.FILTER_RANGE_I64, field=int(f["id"]),
                                                                lo_i=int(body["min"]), hi_i=int(body["max"])))
        elif tag == "F64Range":
            lo, hi = float(body["min"]), float(body["max"])
            if math.isnan(lo) or math.isnan(hi):
                out.append(dict(kind=N.FILTER_OR, arity=0))
            else:
                leaf(out, base, body["field"], "f64", lambda f: dict(kind=N.FILTER_RANGE_F64, field=int(f["id"]),
                                                                    lo_f=lo, hi_f=hi))
        elif tag == "Nested":
            nested_leaf(out, base, body["path"], body["filter"])
        elif tag == "And":
            groups: Dict[str, list] = {}
            plain = 0
            for child in body:
                if isinstance(child, dict) and list(child) == ["Nested"]:
                    groups.setdefault(child["Nested"]["path"], []).append(child["Nested"]["filter"])
                else:
                    walk(out, base, child)
                    plain += 1
            for path, group in groups.items():
                nested_leaf(out, base, path, group[0] if len(group) == 1 else {"And": group})
            out.append(dict(kind=N.FILTER_AND, arity=plain + len(groups)))
        elif tag == "Or":
            for child in body:
                walk(out, base, child)
            out.append(dict(kind=N.FILTER_OR, arity=len(body)))
        elif tag == "Not":
            walk(out, base, body)
            out.append(dict(kind=N.FILTER_NOT))
        else:
            raise ValueError(f"unknown filter {tag!r}")

    top: List[dict] = []
    walk(top, "", filter_json)
    scopes.append((-1, top))
    rows, nodes = [], []
    for path, prog in scopes:
        rows.append((path, len(nodes), len(prog)))
        nodes.extend(prog)
    return NestedFilterProgram(rows, nodes, ords)


def nested_tree_array(trees):
    """trees: NestedFilterProgram objects or (scopes, nodes, ords) triples -> (an N.NestedFilterTree array of
    len(trees) entries (one unused entry when there is none), what it points into)."""
    arr = (N.NestedFilterTree * max(len(trees), 1))()
    keep = []
    names = [n for n, _ in N.FilterNode._fields_]
    for t, tree in enumerate(trees):
        scopes, nodes, ords = (tree.scopes, tree.nodes, tree.ords) if isinstance(tree, NestedFilterProgram) else tree
        sa = (N.NestedScope * max(len(scopes), 1))()
        for i, (path, begin, count) in enumerate(scopes):
            sa[i] = N.NestedScope(int(path), int(begin), int(count))
        na = (N.FilterNode * max(len(nodes), 1))()
        for i, nd in enumerate(nodes):
            unknown = set(nd) - set(names)
            if unknown:
                raise KeyError(f"slg_filter_node has no field {sorted(unknown)}")
            for name, v in nd.items():
                setattr(na[i], name, v)
        oa = np.ascontiguousarray(ords, dtype=np.uint32)
        keep += [sa, na, oa]
        arr[t] = N.NestedFilterTree(len(scopes), C.addressof(sa), len(nodes), C.addressof(na), len(oa),
                                    oa.ctypes.data if len(oa) else None)
    return arr, keep


def nested_columns(fast_fields: Dict[str, dict], n_docs: int) -> dict:
    """The nested columns of ONE segment as index_files.read_fast_fields returns them (NestedCount, NestedParent,
    I64Nested, F64Nested, StrNested) -> what GpuIndex.add_nested_path / add_nested_field / add_nested_keyword_field
    take for that segment: {"paths": {path: {"parent": path one level up or None, "counts": u32[n_docs], "parents":
    (offsets u32[n_docs + 1], values) or None}}, "fields": {name: {"path", "kind": "i64" | "f64" | "keyword",
    "columns": (doc_offsets u32[n_docs + 1], object_offsets, values), "keys": the segment's dictionary (keyword)}}}.
    A column shorter than the segment is padded as the reference reads it (a doc beyond it has no object), a field
    belongs to the longest path that prefixes its name, and a keyword column's values index the SEGMENT's dictionary:
    the caller maps them onto one dictionary over all segments."""
    from .index_files import _I64N, _F64N, _STRN, _NCOUNT, _NPARENT

    def padded_offsets(offs):
        offs = np.asarray(offs, dtype=np.uint32)[:n_docs + 1]
        if len(offs) == 0:
            return np.zeros(n_docs + 1, np.uint32)
        return np.concatenate([offs, np.full(n_docs + 1 - len(offs), offs[-1], np.uint32)])

    out = {"paths": {}, "fields": {}}
    for name, col in fast_fields.items():
        if col["type"] == _NCOUNT and name.startswith("_nested_count:"):
            counts = np.zeros(n_docs, np.uint32)
            v = np.asarray(col["values"], dtype=np.uint32)[:n_docs]
            counts[:len(v)] = v
            out["paths"][name[len("_nested_count:"):]] = {"parent": None, "counts": counts, "parents": None}
    for name, col in fast_fields.items():
        if col["type"] == _NPARENT and name.startswith("_nested_parent:"):
            p = out["paths"].get(name[len("_nested_parent:"):])
            if p is not None:
                p["parents"] = (padded_offsets(col["offsets"]), np.asarray(col["values"], dtype=np.uint32))

    def longest_path(name):
        best = None
        for p in out["paths"]:
            if name.startswith(p + ".") and (best is None or len(p) > len(best)):
                best = p
        return best

    for p, desc in out["paths"].items():
        desc["parent"] = longest_path(p)
    kinds = {_I64N: ("i64", np.int64), _F64N: ("f64", np.float64), _STRN: ("keyword", np.uint32)}
    for name, col in fast_fields.items():
        if col["type"] in kinds and longest_path(name) is not None:
            kind, dt = kinds[col["type"]]
            f = {"path": longest_path(name), "kind": kind,
                 "columns": (padded_offsets(col["doc_offsets"]), np.asarray(col["object_offsets"], dtype=np.uint32),
                             np.asarray(col["values"], dtype=dt))}
            if kind == "keyword":
                f["keys"] = list(col["dict"])
            out["fields"][name] = f
    return out
