"""Numpy restatement of query rescore (api/reader.rs:3238-3398 rescore_hits, :3623-3629
combine_rescore_scores) over the oracle, f32 operation by operation.

  1. First-pass rows = oracle.search_batch / search_batch_filtered / search_batch_min_match at k.
  2. The rescore score r and the matcher = the oracle's exhaustive (brute-force) run of the rescore query (k =
     the docs of all segments): a doc in that result is matched and its score is r; a doc absent from it is not matched.
     The oracle adds a doc's term scores per leaf in term order and the leaves in leaf order, which is the
     order the library fixes.  (The exhaustive run leaves out deleted docs; first-pass rows are live.)
  3. w = min(window, count); a matched row of the first w scores combine(mode, first, r) in f32, the others
     keep their score; the first w rows are sorted by (score desc under total_cmp, segment asc, doc asc); rows
     from w on keep their place.

direct_maps() is step 2 without the oracle's top-k: r of every doc from the oracle's per-posting impacts
(score_tf at weight 1), combined as include/searchlite_gpu.h states it (slg_batch_prepare_rescore, step 3).
It is the reference where an exhaustive top-k run is no fit: negative weights, products that overflow, NaN.

apply_rescore() and direct_maps() are checked by hand-derived cases in tests/test_rescore_ref.py."""
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
    # the brute-force scorer: it adds a leaf's terms in query-term order (the WAND scorer adds them in the order
    # of its cursors, which shows once a leaf has three terms)
    args = (segs, offs, rescore["q_terms"], rescore["q_weights"], k_all)
    if mm is not None and int(np.max(mm, initial=0)) > 1:
        d, s, sc, c = oracle.search_batch_min_match(*args, np.asarray(mm, np.uint32), strategy=oracle.BM25, **plans)
    else:
        d, s, sc, c = oracle.search_batch(*args, strategy=oracle.BM25, **plans)
    return [{(int(s[q, i]), int(d[q, i])): F32(sc[q, i]) for i in range(int(c[q]))} for q in range(nq)]


_impacts = {}


def impacts(oracle, seg, term):
    """(doc ids, f32 impact of every posting of `term` at weight 1): score_tf over the list, df = its length"""
    key = (id(seg), int(term))
    if key not in _impacts:
        a, b = int(seg.term_offsets[term]), int(seg.term_offsets[term + 1])
        f = 0 if seg.term_field is None else int(seg.term_field[term])
        dl, avg = seg.field_doc_len[f], float(seg.field_avgdl[f])
        docs = np.asarray(seg.doc_ids[a:b], np.int64)
        imp = np.array([oracle.score_tf(float(tf), float(b - a), 0.0 if dl is None else float(dl[d]), avg,
                                        float(seg.docs), float(seg.k1), float(seg.b), 1.0)
                        for d, tf in zip(docs, seg.tfs[a:b])], F32)
        _impacts[key] = (seg, docs, imp)  # (the segment is kept: its id stays its own)
    return _impacts[key][1:]


def direct_maps(oracle, segs, rescore):
    """per query {(seg, doc): r} as rescore_maps, from the impacts: a doc's leaf sums start at 0.0 and take
    impact * weight of the leaf's terms in query-term order; a Sum starts at -0.0 and adds the leaves that hold
    the doc in leaf order; a DisMax is m + tie * (sum - m), sum from 0.0, m = the max (f32::max from -inf) of the
    leaves that hold the doc, and of 0.0 if fewer than n_leaves do; matched = at least max(min_match, 1) leaves
    hold the doc.  Every step is one f32 operation."""
    offs = np.asarray(rescore["q_offsets"], np.uint32)
    nq = len(offs) - 1
    terms = np.asarray(rescore["q_terms"], np.uint32).reshape(-1, len(segs))
    weights = np.asarray(rescore["q_weights"], F32)
    leaf_of = rescore.get("q_leaf")
    plan, tie = per_query(rescore.get("q_plan"), nq, 0), per_query(rescore.get("q_tie"), nq, 0.0).astype(F32)
    nleaves, mm = per_query(rescore.get("q_nleaves"), nq, 0), per_query(rescore.get("q_min_match"), nq, 0)
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for q in range(nq):
            t0, t1 = int(offs[q]), int(offs[q + 1])
            leaves = np.arange(t1 - t0) if leaf_of is None else np.asarray(leaf_of, np.int64)[t0:t1]
            n_leaves = max(int(nleaves[q]), int(leaves.max()) + 1 if len(leaves) else 0)
            rmap = {}
            for s, seg in enumerate(segs):
                n = int(seg.n_docs)
                acc = np.full(n, -0.0 if int(plan[q]) == 0 else 0.0, F32)
                mx, nhit = np.full(n, -np.inf, F32), np.zeros(n, np.int64)
                for lf in np.unique(leaves):
                    leafv, hit = np.zeros(n, F32), np.zeros(n, bool)
                    for i in np.nonzero(leaves == lf)[0]:
                        t = int(terms[t0 + i, s])
                        if t == 0xFFFFFFFF:
                            continue
                        docs, imp = impacts(oracle, seg, t)
                        leafv[docs] = leafv[docs] + imp * weights[t0 + i]
                        hit[docs] = True
                    acc[hit] = acc[hit] + leafv[hit]
                    mx[hit] = np.fmax(mx[hit], leafv[hit])
                    nhit += hit
                r = acc
                if int(plan[q]) != 0:
                    m = np.where(nhit < n_leaves, np.fmax(mx, F32(0.0)), mx).astype(F32)
                    r = m + tie[q] * (acc - m)
                assert r.dtype == F32
                for d in np.nonzero(nhit >= max(int(mm[q]), 1))[0]:
                    rmap[(s, int(d))] = F32(r[d])
            out.append(rmap)
    return out


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
