"""Numpy restatement of hybrid text + vector search (api/reader.rs:2754-2775: collect_vector_maps with
require_text_match = true, :2379-2469, then merge_vector_hits, :2474-2537), f32 operation by operation.

  1. M = the docs the text query matches (not deleted, passing the filter): oracle.search_batch* at k = all docs.
  2. BM25 hits = the first k of M (score desc, segment asc, doc asc).
  3. Clause list c = the best cand_size of {metric_similarity * boost : doc in M with a vector in the field} by
     (score desc, segment asc, doc asc); similarities from oracle.rerank at alpha 0, the boost an f32 multiply.
  4. union = BM25 hits + lists; bm25 = the hit's score or 0.0; compute_hybrid_score (:225-254); the
     all_vector_only drop (:2494,2504).
  5. top k_out by (final desc under total_cmp, segment asc, doc asc).

clause_list() and merge_vector_hits() are pure (tests/test_hybrid_ref.py checks them by hand-derived cases)."""
import numpy as np

F32 = np.float32
NOVEC = 0xFFFFFFFF
F32_MIN = F32(np.finfo(np.float32).min)


def tkey(x):
    """f32::total_cmp key"""
    b = int(np.array(x, F32).view(np.int32))
    return b ^ 0x7FFFFFFF if b < 0 else b


def missing(metric):
    return F32(-1.0) if metric == 0 else F32_MIN


NEAR = 4e-5  # scores this close to a boundary's two scores belong to its near-tie


def clause_list(entries, cand):
    """entries [(score, seg, doc)] -> ({(seg, doc): score} of the best cand, the gap at the boundary or inf)"""
    ents = sorted(entries, key=lambda e: (-tkey(e[0]), e[1], e[2]))
    gap = np.inf
    if len(ents) > cand:
        gap = abs(float(ents[cand - 1][0]) - float(ents[cand][0]))
    return {(s, d): F32(v) for v, s, d in ents[:cand]}, gap


def boundary_keys(entries, cut):
    """the (seg, doc) of the entries [(score, seg, doc)] whose score lies within NEAR of the two scores at the
    cut of the sorted list (empty when the list is not cut): the docs a near-tie at the cut may move"""
    ents = sorted(entries, key=lambda e: (-tkey(e[0]), e[1], e[2]))
    if not 0 < cut < len(ents):
        return set()
    lo, hi = float(ents[cut][0]), float(ents[cut - 1][0])
    return {(s, d) for v, s, d in ents if lo - NEAR <= float(v) <= hi + NEAR}


def hybrid_score(key, bm25, alpha, metrics, maps):
    """compute_hybrid_score: (final, vector score or None)"""
    bsum, vsum, has = F32(0.0), F32(0.0), False
    with np.errstate(over="ignore", invalid="ignore"):
        for c, m in enumerate(maps):
            if key in m:
                vs = m[key]
                vsum = F32(vsum + vs)
                has = True
            else:
                vs = missing(metrics[c])
            a = F32(alpha[c])
            if a >= 1:
                bl = F32(bm25)
            elif a <= 0:
                bl = vs
            else:
                bl = F32(F32(a * F32(bm25)) + F32(F32(F32(1.0) - a) * vs))
            bsum = F32(bsum + bl)
        return F32(bsum / F32(len(maps))), (vsum if has else None)


def merge_vector_hits(bm25_hits, maps, alpha, metrics, k_out):
    """bm25_hits [(seg, doc, score)], maps = the clause lists -> (rows [(seg, doc, final, vec or None)] of the
    top k_out, the union size after the all_vector_only drop, the gap of the finals at the k_out boundary)"""
    bm = {(s, d): F32(v) for s, d, v in bm25_hits}
    union = set(bm).union(*[m.keys() for m in maps]) if maps else set(bm)
    vec_only = all(F32(a) <= 0 for a in alpha)
    rows = []
    for key in union:
        fin, vec = hybrid_score(key, bm.get(key, F32(0.0)), alpha, metrics, maps)
        if vec_only and vec is None:
            continue
        rows.append((key[0], key[1], fin, vec))
    rows.sort(key=lambda r: (-tkey(r[2]), r[0], r[1]))
    gap = np.inf
    if 0 < k_out < len(rows):
        gap = abs(float(rows[k_out - 1][2]) - float(rows[k_out][2]))
    return rows[:k_out], len(rows), gap


def matched(oracle, segs, q_offsets, q_terms, q_weights, q_filter=None, filters=None, strategy=0, **plans):
    """per query [(seg, doc, score)] of every matched doc in (score desc, seg, doc) order"""
    n_all = max(sum(s.n_docs for s in segs), 1)
    if q_filter is not None:
        r = oracle.search_batch_filtered(segs, q_offsets, q_terms, q_weights, n_all, q_filter, filters,
                                         strategy=strategy, **plans)
    else:
        r = oracle.search_batch(segs, q_offsets, q_terms, q_weights, n_all, strategy=strategy, **plans)
    doc, seg, score, count = r[:4]
    return [[(int(seg[q, i]), int(doc[q, i]), F32(score[q, i])) for i in range(int(count[q]))]
            for q in range(len(count))]


def reference(oracle, segs, fields, clause_field, q_offsets, q_terms, q_weights, k, qvecs, alpha, boost, cand,
              k_out, q_filter=None, filters=None, strategy=0, **plans):
    """fields[f][s] = (metric, offsets, values) or None.  -> per query dict(rows, total, bm25 (the hits),
    gap (the smallest gap at a clause's cand boundary or at the k_out boundary; exact ties count as inf),
    near (the docs within NEAR of a clause's cand boundary or of the k_out boundary))"""
    nq, nc = len(q_offsets) - 1, len(clause_field)
    alpha = np.broadcast_to(np.asarray(alpha, F32), (nq, nc))
    boost = np.ones((nq, nc), F32) if boost is None else np.broadcast_to(np.asarray(boost, F32), (nq, nc))
    metrics = [next(st[0] for st in fields[f] if st is not None) for f in clause_field]
    dims = [next(st[2].shape[1] for st in fields[f] if st is not None) for f in clause_field]
    offs = np.concatenate([[0], np.cumsum(dims)]).astype(int)
    M = matched(oracle, segs, q_offsets, q_terms, q_weights, q_filter, filters, strategy, **plans)
    out = []
    for q in range(nq):
        hits = M[q][:k]
        maps, gap, near = [], np.inf, set()
        for c, f in enumerate(clause_field):
            ents = []
            for s, st in enumerate(fields[f]):
                if st is None:
                    continue
                metric, vo, vals = st
                docs = np.array(sorted(d for sg, d, _ in M[q] if sg == s and d < len(vo) and vo[d] != NOVEC), np.uint32)
                if len(docs) == 0:
                    continue
                od, _, ov = oracle.rerank(metric, vo, vals, qvecs[q, offs[c]:offs[c + 1]], 0.0, docs,
                                          np.zeros(len(docs), F32), len(docs))
                with np.errstate(over="ignore", invalid="ignore"):
                    ents += [(F32(F32(v) * boost[q, c]), s, int(d)) for d, v in zip(od, ov)]
            m, g = clause_list(ents, cand)
            maps.append(m)
            gap = min(gap, g if g > 0 else np.inf)
            near |= boundary_keys(ents, cand)
        rows, total, g = merge_vector_hits(hits, maps, alpha[q], metrics, k_out)
        every, _, _ = merge_vector_hits(hits, maps, alpha[q], metrics, total)
        near |= boundary_keys([(r[2], r[0], r[1]) for r in every], k_out)
        out.append(dict(rows=rows, total=total, bm25=hits, gap=min(gap, g if g > 0 else np.inf), maps=maps,
                        near=near))
    return out
