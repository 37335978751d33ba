"""The reference of a compound request (slg_batch_prepare_request), composed from the references of its kinds in the
order the reference runs them per candidate (query/wand.rs:506-517): score_adjust (which may drop the doc), then
accept (tombstones, matcher, root filter, cursor, matched count), then collector.collect; rescore and collapse
work on the finished rows (api/reader.rs:3238-3398, 3499-3562).

  1. candidates  fscore_ref.all_candidates(): the oracle's exhaustive run over tombstone-free copies of the segments,
                 every doc of the scored lists with its exact first-pass score.
  2. clause      the pass mask of bool_ref / phrase_ref / booltree_ref per (query, segment) — the mask those
                 references hand the oracle as the query's filter — takes the rejected candidates out.  The matcher
                 reads no score and the score stage reads no matcher, so taking them out first keeps exactly the docs
                 score_adjust-then-matcher keeps.
  3. score       script_ref.apply(): the query's chain of function_score / script_score stages over the survivors
                 (fscore_ref.evaluate, script_ref.evaluate_docs), tombstones and the query's own filter after it.
                 What the clause and the score stage leave is `scored_docs`; the live docs among them that pass the
                 filter are the MATCHED SET, each with its rewritten score, ranked by score.
  4. order       the matched set under the request's sort (collapse_ref.sort_key: the full SortKey), cut behind the
                 cursor's row (the docs strictly after it; `seen`: the cursor's doc is in the set) and at k.
  5. collectors  agg_date_ref (every aggregation kind), top_hits_ref, composite_ref, term_buckets_ref over the
                 matched set; collapse_ref over the rows; rescore_ref.rescore_batch over the rows.

Nothing here is new arithmetic: every number comes from one of the references named above, each of which is checked
against hand-derived tables in its own test file.  What this module adds is the order of composition, which
tests/test_request_ref.py checks against hand-derived tables of its own."""
import numpy as np

from tests import agg_date_ref, bool_ref, booltree_ref, collapse_ref, composite_ref, fscore_ref, phrase_ref
from tests import rescore_ref, script_ref, term_buckets_ref, top_hits_ref

F32 = np.float32
SCORE_DESC = collapse_ref.SCORE_DESC


def clause_masks(segs, nq, clause, tree_filters=None):
    """clause: None, ("bool", clauses), ("phrase", phrases, clauses or None) or ("bool_tree", descriptions)
    -> per query None (no matcher: untouched) or [pass mask per segment]"""
    if clause is None:
        return [None] * nq
    kind = clause[0]
    if kind == "bool":
        return bool_ref.clause_masks(segs, clause[1])
    if kind == "phrase":
        return phrase_ref.clause_masks(segs, clause[2], clause[1])
    if kind == "bool_tree":
        return booltree_ref.nested_masks(segs, clause[1], tree_filters)
    raise ValueError(kind)


def keep_candidates(cands, masks):
    """the candidates a clause stage leaves: rows compacted per query, in their order -> (doc, seg, score, count)"""
    doc, seg, score, count = cands
    out = (np.zeros_like(doc), np.zeros_like(seg), np.zeros_like(score), np.zeros_like(count))
    for q in range(len(count)):
        n = int(count[q])
        keep = np.ones(n, bool)
        if masks[q] is not None:
            for s, m in enumerate(masks[q]):
                at = np.nonzero(seg[q, :n] == s)[0]
                keep[at] = np.asarray(m, bool)[doc[q, at].astype(np.int64)]
        at = np.nonzero(keep)[0]
        out[0][q, :len(at)], out[1][q, :len(at)], out[2][q, :len(at)], out[3][q] = doc[q, at], seg[q, at], score[q, at], len(at)
    return out


def matched_sets(cands, segs, nq, clause=None, chains=None, cols=None, q_filter=None, tree_filters=None):
    """steps 2 and 3 -> dict(rows = per query the matched set [(seg, doc, score)] in score order, scored = scored_docs
    [nq], matched [nq], clause_kept = candidates behind the clause stage [nq])"""
    kept = keep_candidates(cands, clause_masks(segs, nq, clause, tree_filters))
    cols = fscore_ref.Columns(segs) if cols is None else cols
    chains = [[] for _ in range(nq)] if chains is None else chains
    k_all = max(int(cands[0].shape[1]), 1)
    _, scored, matched, rows = script_ref.apply(kept, segs, chains, cols, k_all, q_filter)
    return dict(rows=rows, scored=scored, matched=matched, clause_kept=np.asarray(kept[3], np.uint64))


def chains_of(nq, fscore=None, script=None, order="outer"):
    """per query the stages in the order they run (script_order outer: script_score{query: function_score})"""
    out = []
    for q in range(nq):
        stages = [] if script is None else [("script", script[q])]
        if fscore is not None:
            fs = ("fscore", fscore[q])
            stages = [fs] + stages if order == "outer" else stages + [fs]
        out.append(stages)
    return out


def ordered(rows, sort=None, fields=None):
    """step 4, the order: per query the matched set under `sort` ([(part, order)], part "_score" or a name in
    `fields`; None: score order, as the rows are).  A sort without a `_score` part leaves the scores 0.0
    (ScoreMode::MatchOnly)"""
    if sort is None:
        return [list(h) for h in rows]
    out = []
    for hits in rows:
        hits = sorted(hits, key=collapse_ref.sort_key(sort, fields))
        if not any(p == "_score" for p, _ in sort):
            hits = [(s, d, F32(0.0)) for s, d, _ in hits]
        out.append(hits)
    return out


def cursor_of(hit, sort, fields):
    """the cursor that names a row: (values per sort part, segment, doc), as GpuIndex.search_after takes it"""
    s, d, sc = hit
    vals = tuple(float(sc) if p == "_score" else collapse_ref.pick(fields[p][0][s][d], o) for p, o in (sort or SCORE_DESC))
    return vals, s, d


def paged(rows, after, sort=None, fields=None):
    """step 4, the cursor: after[q] = None (a first page) or the rank behind which query q's page starts
    -> (cursors per query, the rows behind them, matched [nq] = their number, seen [nq])"""
    cursors, out = [], []
    for hits, a in zip(rows, after):
        if a is None or a == 0:
            cursors.append(None)
            out.append(list(hits))
        else:
            assert 0 < a <= len(hits), "the cursor must name a row of the matched set"
            cursors.append(cursor_of(hits[a - 1], sort, fields))
            out.append(list(hits[a:]))
    return cursors, out, np.array([len(h) for h in out], np.uint64), np.ones(len(out), np.uint8)


def as_arrays(rows, k):
    """per query rows cut at k -> (doc, seg, score [nq, k], count [nq]) as slg_batch_fetch returns them"""
    nq = len(rows)
    doc, seg = np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.uint32)
    score, count = np.zeros((nq, k), F32), np.zeros(nq, np.uint32)
    for q, hits in enumerate(rows):
        hits = hits[:k]
        count[q] = len(hits)
        for i, (s, d, sc) in enumerate(hits):
            seg[q, i], doc[q, i], score[q, i] = s, d, sc
    return doc, seg, score, count


def docs_of(rows):
    return [[(s, d) for s, d, _ in hits] for hits in rows]


# ---- step 5: the collectors over the matched set, rescore and collapse over the rows ---------------------------------
def agg_tables(request, nodes, cols, masks, keys_of, rows):
    """agg_date_ref over the matched set -> (layout, dense tables per node [nq, parent_rows, rows], responses)"""
    layout = agg_date_ref.ref_layout(nodes, cols, keys_of)
    states = [agg_date_ref.run(request, cols, masks, d) for d in docs_of(rows)]
    per_q = [agg_date_ref.dense(nodes, layout, st, keys_of) for st in states]
    tables = [np.stack([t[i] for t in per_q]) for i in range(len(nodes))]
    return layout, tables, [agg_date_ref.respond(request, st) for st in states]


def top_hits_root(rows, size, frm=0, sort=(), fields=None):
    """a root top_hits node: one list per query over the matched set with its rewritten scores
    -> [per query [(seg, doc, score)]]"""
    return [top_hits_ref.one_list(list(hits), size, frm, list(sort), fields) for hits in rows]


def composite_page(body, cols, f64_fields, rows, after=None):
    """composite_ref over the matched set -> per query (bucket rows [(key, docs)], has_more)"""
    out = []
    for d in docs_of(rows):
        buckets = composite_ref.collect(body["sources"], cols, f64_fields, d)
        out.append(composite_ref.finalize(body["sources"], buckets, body["size"], after))
    return out


def term_bucket_responses(body, cols, n_docs, deleted, masks, rows):
    return [term_buckets_ref.respond(body, cols, n_docs, deleted, masks, d, False) for d in docs_of(rows)]


def collapse_arrays(page, column, spec, main_sort=None, fields=None):
    """collapse_ref over the rows (doc, seg, score, count); spec: group_limit, inner_from, inner_size, inner_sort
    by field names"""
    return collapse_ref.expected_arrays(*page, column, spec["group_limit"], spec.get("inner_from", 0),
                                        spec.get("inner_size", 0), spec.get("inner_sort"), main_sort, fields)


def rescored(page, maps, window, mode=None):
    """rescore_ref over the rows -> (doc, seg, score, count, first_score, rescore_score, rescored)"""
    return rescore_ref.rescore_batch(page, maps, window, mode)
