"""Unscored root queries for slg_batch_prepare_scan: match_all, constant_score and rank_feature dictionaries, as a
search request states them, shaped into the per-query arrays of slg_scan_spec.

A query is one of
    {"match_all": {}}                                            score 1.0
    {"constant_score": {"filter": f, "boost": b}}                score b (default 1.0) * node_boost
    {"rank_feature": {"field": id, "modifier": m, "missing": x, "boost": b}}
with f a registered filter id (add_filter*) or None, id a numeric agg field id (add_agg_field), m one of None,
"none", "log", "log1p", "sqrt", "reciprocal" (or a SCAN_MOD_* number), missing default 0.0 and boost default 1.0.
Every form takes "node_boost" (default 1.0), the boost the node itself carries: the ABI takes final values, so
constant_score's score is boost * node_boost and rank_feature's boost is boost * node_boost, multiplied here in
f32 as the reference's planner does.  A match_all may carry "filter" too (a bool query that is nothing but filters).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N

MODIFIERS = {None: N.SCAN_MOD_NONE, "none": N.SCAN_MOD_NONE, "log": N.SCAN_MOD_LOG, "log1p": N.SCAN_MOD_LOG1P,
             "sqrt": N.SCAN_MOD_SQRT, "reciprocal": N.SCAN_MOD_RECIPROCAL}


def scan_arrays(queries) -> dict:
    """queries: one dictionary per query -> the arrays of slg_scan_spec by field name."""
    nq = len(queries)
    a = dict(q_kind=np.zeros(nq, np.int32), q_filter=np.full(nq, -1, np.int32), q_score=np.ones(nq, np.float32),
             q_field=np.zeros(nq, np.int32), q_modifier=np.zeros(nq, np.int32), q_missing=np.zeros(nq, np.float32),
             q_boost=np.ones(nq, np.float32))
    for q, query in enumerate(queries):
        if len(query) != 1:
            raise ValueError(f"query {q}: exactly one of match_all, constant_score, rank_feature")
        (name, body), = query.items()
        body = body or {}
        node_boost = np.float32(body.get("node_boost", 1.0))
        flt = body.get("filter")
        a["q_filter"][q] = -1 if flt is None else int(flt)
        if name == "match_all":
            a["q_kind"][q] = N.SCAN_MATCH_ALL
        elif name == "constant_score":
            a["q_kind"][q] = N.SCAN_CONSTANT
            a["q_score"][q] = np.float32(body.get("boost", 1.0)) * node_boost
        elif name == "rank_feature":
            a["q_kind"][q] = N.SCAN_RANK_FEATURE
            a["q_field"][q] = int(body["field"])
            m = body.get("modifier")
            a["q_modifier"][q] = MODIFIERS[m] if m in MODIFIERS else int(m)
            a["q_missing"][q] = np.float32(body.get("missing", 0.0))
            a["q_boost"][q] = np.float32(body.get("boost", 1.0)) * node_boost
        else:
            raise ValueError(f"query {q}: unknown unscored query `{name}`")
    return a


def scan_spec(queries):
    """-> (N.ScanSpec, the arrays it points into: keep them alive as long as the spec is used)"""
    keep = scan_arrays(queries)
    spec = N.ScanSpec(*[keep[name].ctypes.data_as(C.c_void_p) for name, _ in N.ScanSpec._fields_])
    return spec, keep
