"""The arrays of PreparedBatch.explain (slg_batch_explain) in the reference's JSON form: HitExplanation
(api/reader.rs:90-97) per explained row.

shape(arrays, field_names, counts=None) -> per query a list of dicts, one per explained row:
    {"base_score": f, "functions": [{"type": s, "value": f[, "field": name]}], "final_score": f
     [, "rescore": {"rescore_score": f, "combined_score": f, "functions": []}]}
`type` is one of TYPE_NAMES; `field` is the name the caller gives the agg field id (field_names: a dict or a
callable), absent for a weight and a script; `rescore` is present only for a row the rescore query matched (a rescore
batch takes no score stage, so its function list is empty).  counts: the batch's row counts (fetch()[3]); the rows of
query q are the first min(rows, counts[q]).  Without counts every row of the arrays is shaped."""
import numpy as np

from . import _native as N

TYPE_NAMES = {N.EXPLAIN_WEIGHT: "weight", N.EXPLAIN_FIELD_VALUE_FACTOR: "field_value_factor",
              N.EXPLAIN_DECAY_EXP: "decay_exp", N.EXPLAIN_DECAY_GAUSS: "decay_gauss",
              N.EXPLAIN_DECAY_LINEAR: "decay_linear", N.EXPLAIN_SCRIPT_SCORE: "script_score"}


def shape(arrays, field_names, counts=None):
    name_of = field_names if callable(field_names) else field_names.__getitem__
    base, final, n_fn = arrays["base_score"], arrays["final_score"], arrays["n_functions"]
    nq, rows = base.shape
    out = []
    for q in range(nq):
        n = rows if counts is None else min(rows, int(counts[q]))
        hits = []
        for r in range(n):
            functions = []
            for e in range(int(n_fn[q, r])):
                entry = {"type": TYPE_NAMES[int(arrays["fn_type"][q, r, e])], "value": float(arrays["fn_value"][q, r, e])}
                field = int(arrays["fn_field"][q, r, e])
                if field >= 0:
                    entry["field"] = name_of(field)
                functions.append(entry)
            hit = {"base_score": float(base[q, r]), "functions": functions, "final_score": float(final[q, r])}
            if "rescored" in arrays and int(arrays["rescored"][q, r]):
                hit["rescore"] = {"rescore_score": float(arrays["rescore_score"][q, r]),
                                  "combined_score": float(arrays["combined_score"][q, r]), "functions": []}
            hits.append(hit)
        out.append(hits)
    return out
