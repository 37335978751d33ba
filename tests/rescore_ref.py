"""Numpy restatement of query rescore (api/reader.rs:3238-3398 rescore_hits, :3623-3629
combine_rescore_scores) over the oracle, f32 operation by operation.

  1. First-pass rows = oracle.search_batch / search_batch_filtered / search_batch_min_match at k.
  2. The rescore score r and the matcher = the oracle's exhaustive run of the rescore query (k = the docs of
     all segments): a doc in that result is matched and its score is r; a doc absent from it is not matched.
     The oracle adds a doc's term scores per leaf in term order and the leaves in leaf order, which is the
     order the library fixes.  (The exhaustive run leaves out deleted docs; first-pass rows are live.)
  3. w = min(window, count); a matched row of the first w scores combine(mode, first, r) in f32, the others
     keep their score; the first w rows are sorted by (score desc under total_cmp, segment asc, doc asc); rows
     from w on keep their place.

apply_rescore() is pure (tests/test_rescore_ref.py checks it by hand-derived cases)."""
import numpy as np

from tests.util import _f32_key

F32 = np.float32
TOTAL, MULTIPLY, SUM, MAX, MIN = 0, 1, 2, 3, 4


def combine(mode, o, r):
    """combine_rescore_scores: plain f32 operations (f32::max / f32::min: a NaN operand yields the other)"""
    o, r = F32(o), F32(r)
    with np.errstate(over="ignore", invalid="ignore"):
        if mode == MULTIPLY:
            return F32(o * r)
        if mode == MAX:
            return F32(np.fmax(o, r))
        if mode == MIN:
            return F32(np.fmin(o, r))
        return F32(o + r)


def apply_rescore(doc, seg, score, count, r_map, window, mode):
    """One query.  doc / seg / score: its first-pass rows [k]; r_map: {(seg, doc): r} of the docs the rescore
    query matches (None or empty: it matches nothing, or has no term)
    -> (doc, seg, score, first_score, rescore_score, rescored), each [k]."""
    k = len(doc)
    doc, seg, score = np.array(doc, np.uint32), np.array(seg, np.uint32), np.array(score, F32)
    first, rsc, flag = score.copy(), np.zeros(k, F32), np.zeros(k, np.uint32)
    w = min(int(window), int(count))
    if w == 0 or not r_map:
        return doc, seg, score, first, rsc, flag
    for i in range(w):
        r = r_map.get((int(seg[i]), int(doc[i])))
        if r is not None:
            rsc[i] = F32(r)
            flag[i] = 1
            score[i] = combine(mode, first[i], r)
    order = np.lexsort((doc[:w], seg[:w], -_f32_key(score[:w])))
    for a in (doc, seg, score, first, rsc, flag):
        a[:w] = a[:w][order]
    return doc, seg, score, first, rsc, flag


def first_pass(oracle, segs, q_offsets, q_terms, q_weights, k, q_filter=None, filters=None, q_min_match=None, **plans):
    if q_min_match is not None:
        return oracle.search_batch_min_match(segs, q_offsets, q_terms, q_weights, k, q_min_match,
                                             q_filter=q_filter, filters=filters, **plans)
    if q_filter is not None:
        return oracle.search_batch_filtered(segs, q_offsets, q_terms, q_weights, k, q_filter, filters, **plans)
    return oracle.search_batch(segs, q_offsets, q_terms, q_weights, k, **plans)


def rescore_maps(oracle, segs, rescore):
    """per query {(seg, doc): r}: the exhaustive run of the rescore queries (rescore: the dict of
    GpuIndex.search_rescore)"""
    k_all = int(sum(s.n_docs for s in segs))
    plans = {n: rescore[n] for n in ("q_leaf", "q_plan", "q_tie", "q_nleaves") if rescore.get(n) is not None}
    offs = np.asarray(rescore["q_offsets"], np.uint32)
    nq = len(offs) - 1
    for n in ("q_plan", "q_tie", "q_nleaves"):
        if n in plans and np.ndim(plans[n]) == 0:
            plans[n] = np.full(nq, plans[n])
    mm = rescore.get("q_min_match")
    if mm is not None and np.ndim(mm) == 0:
        mm = np.full(nq, mm)
    args = (segs, offs, rescore["q_terms"], rescore["q_weights"], k_all)
    if mm is not None and int(np.max(mm, initial=0)) > 1:
        d, s, sc, c = oracle.search_batch_min_match(*args, np.asarray(mm, np.uint32), **plans)
    else:
        d, s, sc, c = oracle.search_batch(*args, **plans)
    return [{(int(s[q, i]), int(d[q, i])): F32(sc[q, i]) for i in range(int(c[q]))} for q in range(nq)]


def per_query(x, nq, default):
    if x is None:
        x = default
    return np.full(nq, x) if np.ndim(x) == 0 else np.asarray(x)


def rescore_batch(first, maps, window, mode=None):
    """first = (doc, seg, score, count) of the first pass; maps = rescore_maps(...)
    -> (doc, seg, score, count, first_score, rescore_score, rescored)"""
    doc, seg, score, count = first
    nq = len(count)
    window, mode = per_query(window, nq, 0), per_query(mode, nq, TOTAL)
    out = [apply_rescore(doc[q], seg[q], score[q], count[q], maps[q], window[q], int(mode[q])) for q in range(nq)]
    stack = lambda i: np.stack([o[i] for o in out]) if nq else np.zeros((0, doc.shape[1]), out_dtypes[i])
    out_dtypes = (np.uint32, np.uint32, F32, F32, F32, np.uint32)
    return stack(0), stack(1), stack(2), np.asarray(count), stack(3), stack(4), stack(5)


def reference(oracle, segs, q_offsets, q_terms, q_weights, k, rescore, q_filter=None, filters=None, **plans):
    first = first_pass(oracle, segs, q_offsets, q_terms, q_weights, k, q_filter=q_filter, filters=filters, **plans)
    return rescore_batch(first, rescore_maps(oracle, segs, rescore), rescore["window"], rescore.get("mode"))
