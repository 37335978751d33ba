"""Numpy restatement of explain (SearchRequest.explain; HitExplanation, api/reader.rs:90-97) in the flat form of
slg_batch_explain, built on tests/fscore_ref.py, tests/script_ref.py and tests/rescore_ref.py.

Per ranked row (segment, doc) of a query:
  base     the first-pass score of the doc before any score stage: ScorePlan::evaluate(leaves), looked up in the
           oracle's exhaustive run (fscore_ref.all_candidates)
  entries  [(type, field, value f32)] in the order evaluate_compiled_score appends them (:418-613): the stages of the
           query's chain in the order they run (inner node first).  A function_score stage appends one entry per
           function that gives the doc a value, in request order (describe_function, :389-416): type TYPE of the
           function, field = the function's field (None for a weight); a function whose filter rejects the doc, a
           decay without a value, a non-finite field_value_factor: nothing.  A script_score stage appends
           ("script_score", None, script * boost).  A stage whose query entry is None appends nothing.
  final    the end of the chain: each stage reads the score the stage before it left (fscore_ref.evaluate /
           script_ref.evaluate_docs).  base itself is never rewritten: the `eff = 1.0` substitution of a base within
           f32 epsilon of 0 only enters the stage's result.
A rescore batch has no stage: base is the first-pass score (first_score), final the row's score after the rescore,
and the rescore part (rescore_score, combined_score) exists for a row the rescore query matched inside the window.

The reference is checked against a literal transcription of the recursion and hand-derived cases in
tests/test_explain_ref.py."""
import numpy as np

from tests import fscore_ref, script_ref

F32 = np.float32
TYPES = ("weight", "field_value_factor", "decay_exp", "decay_gauss", "decay_linear", "script_score")


def function_type(fn):
    return "decay_" + fn.get("function", "exp") if fn["kind"] == "decay" else fn["kind"]


def base_lookup(cands):
    """fscore_ref.all_candidates() -> per query {(seg, doc): f32 first-pass score}"""
    doc, seg, score, count = cands
    return [{(int(seg[q, i]), int(doc[q, i])): F32(score[q, i]) for i in range(int(count[q]))} for q in range(len(count))]


def explain_rows(chain, cols, rows, base):
    """one query: chain = [("script", entry) | ("fscore", spec)] in the order the stages run; rows = [(seg, doc)];
    base = f32 per row -> [dict(base=, entries=[(type, field or None, f32)], final=)]"""
    out = [dict(base=F32(b), entries=[], final=F32(b)) for b in base]
    segs = np.array([s for s, _ in rows], np.int64)
    for s in np.unique(segs):  # (the references work on the docs of one segment at a time)
        at = np.nonzero(segs == s)[0]
        docs = np.array([rows[i][1] for i in at], np.int64)
        cur = np.array([base[i] for i in at], F32)
        for kind, spec in chain:
            if spec is None:
                continue
            if kind == "fscore":
                for fn in spec.get("functions", ()):
                    val, has, _ = fscore_ref.function_value(fn, cols, int(s), docs)
                    entry = (function_type(fn), None if fn["kind"] == "weight" else fn["field"])
                    for j in np.nonzero(has)[0]:
                        out[at[j]]["entries"].append(entry + (F32(val[j]),))
                cur, _ = fscore_ref.evaluate(spec, cols, int(s), docs, cur)
            else:
                assert kind == "script", kind
                cur, _ = script_ref.evaluate_docs(spec, cols, int(s), docs, cur)
                for j in range(len(at)):
                    out[at[j]]["entries"].append(("script_score", None, F32(cur[j])))
        for j in range(len(at)):
            out[at[j]]["final"] = F32(cur[j])
    return out


def explain(cands, chains, cols, rows):
    """cands: fscore_ref.all_candidates(); chains[q]; rows[q] = [(seg, doc)] -> per query explain_rows()"""
    look = base_lookup(cands)
    return [explain_rows(chains[q], cols, rows[q], [look[q][r] for r in rows[q]]) for q in range(len(rows))]


def explain_rescore(rescored_rows, n):
    """one query of a rescore batch: rescored_rows = (doc, seg, score, first_score, rescore_score, rescored) as
    rescore_ref.apply_rescore returns them; n rows -> [dict(base=, entries=[], final=, rescore=None | dict)]"""
    doc, seg, score, first, rsc, flag = rescored_rows
    out = []
    for i in range(n):
        part = dict(rescore_score=F32(rsc[i]), combined_score=F32(score[i])) if int(flag[i]) else None
        out.append(dict(base=F32(first[i]), entries=[], final=F32(score[i]), rescore=part))
    return out


def as_arrays(per_query, rows, field_id=lambda f: f, n_funcs=9, with_rescore=False):
    """the per-query lists in the layout of slg_explain_out at a stride of `rows` (zeros behind a query's rows)"""
    nq = len(per_query)
    out = dict(base_score=np.zeros((nq, rows), F32), final_score=np.zeros((nq, rows), F32),
               n_functions=np.zeros((nq, rows), np.uint32), fn_type=np.zeros((nq, rows, n_funcs), np.uint32),
               fn_field=np.zeros((nq, rows, n_funcs), np.int32), fn_value=np.zeros((nq, rows, n_funcs), F32))
    if with_rescore:
        out.update(rescored=np.zeros((nq, rows), np.uint32), rescore_score=np.zeros((nq, rows), F32),
                   combined_score=np.zeros((nq, rows), F32))
    for q, hits in enumerate(per_query):
        for r, h in enumerate(hits[:rows]):
            out["base_score"][q, r], out["final_score"][q, r] = h["base"], h["final"]
            out["n_functions"][q, r] = len(h["entries"])
            for e, (typ, field, val) in enumerate(h["entries"]):
                out["fn_type"][q, r, e] = TYPES.index(typ)
                out["fn_field"][q, r, e] = -1 if field is None else field_id(field)
                out["fn_value"][q, r, e] = val
            if with_rescore and h.get("rescore"):
                out["rescored"][q, r] = 1
                out["rescore_score"][q, r] = h["rescore"]["rescore_score"]
                out["combined_score"][q, r] = h["rescore"]["combined_score"]
    return out
