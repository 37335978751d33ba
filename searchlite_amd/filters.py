"""Filter trees for the device (slg_index_add_filter_trees): request -> postfix program.

The reference's `filter` (api/types.rs: KeywordEq, KeywordIn, I64Range, F64Range, Nested, And, Or, Not, in serde's
externally tagged JSON form, e.g. {"And": [{"KeywordEq": {"field": "cat", "value": "news"}}, ...]}) is evaluated per
doc by query/filters.rs over the fast fields.  The device evaluates the same tree over the columns registered with
GpuIndex.add_agg_field / add_agg_keyword_field; what is host work lives here: walking the JSON into postfix order
and resolving keyword strings to the ordinals of the column's dictionary with the reference's
case_insensitive_equals (index/fastfields.rs:475-481), under which several dictionary keys may equal one value.

A leaf the reference answers `false` for every doc (a field that does not exist, or one of another kind:
fastfields.rs `_ => false`; an F64Range with a NaN bound) compiles to OR of nothing, which is false.
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
