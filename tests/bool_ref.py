"""Numpy restatement of the boolean matcher's accept() (QueryEvaluator::matches_node, api/reader.rs:1485-1565;
term_group_matches, :1571-1580) in the flat form of slg_batch_prepare_bool, over the oracle.

  1. clause_masks(): per (query, segment) one boolean pass mask over the segment's docs, straight from the posting
     arrays: a group holds a doc if any of its terms has a posting of it; a doc passes iff every MUST group holds
     it, no MUST_NOT group does, and at least min_should SHOULD groups do.  None for a query without a group.
  2. reference(): oracle.search_batch_filtered with that mask as the query's filter, AND-ed with the query's own
     filter mask where it has one — the reference's accept = !deleted && matcher.matches(doc) && filter.
  3. scored_docs(): the docs of the scored lists (tombstoned ones included, as slg_stats counts them) the clause
     mask passes.

clauses_of() builds the spec's arrays from a per-query description.  The mask builder is checked by hand-derived
cases in tests/test_bool_ref.py."""
import numpy as np

MUST, SHOULD, MUST_NOT = 0, 1, 2
NO_TERM = 0xFFFFFFFF


def clauses_of(queries, n_segs):
    """queries: per query (groups, min_should), groups = [(kind, [term, ...])], term = one id for every segment or
    a sequence of one id per segment (NO_TERM where absent) -> the dict of GpuIndex.search_batch_bool"""
    c_offsets, c_terms, c_group, g_offsets, g_kind, min_should = [0], [], [], [0], [], []
    for groups, ms in queries:
        for g, (kind, terms) in enumerate(groups):
            g_kind.append(kind)
            for t in terms:
                c_terms.append([t] * n_segs if np.ndim(t) == 0 else list(t))
                c_group.append(g)
        c_offsets.append(len(c_group))
        g_offsets.append(len(g_kind))
        min_should.append(ms)
    return dict(c_offsets=np.array(c_offsets, np.uint32), c_terms=np.array(c_terms, np.uint32).reshape(-1, n_segs),
                c_group=np.array(c_group, np.uint32), g_offsets=np.array(g_offsets, np.uint32),
                g_kind=np.array(g_kind, np.int32), q_min_should=np.array(min_should, np.uint32))


def postings(seg, term):
    return np.asarray(seg.doc_ids[int(seg.term_offsets[term]):int(seg.term_offsets[term + 1])], np.int64)


def clause_masks(segs, clauses):
    """-> per query None (no group: untouched) or [one bool mask per segment]"""
    c_off, g_off = np.asarray(clauses["c_offsets"], np.int64), np.asarray(clauses["g_offsets"], np.int64)
    terms = np.asarray(clauses["c_terms"], np.uint32).reshape(-1, len(segs))
    group, kind = np.asarray(clauses["c_group"], np.int64), np.asarray(clauses["g_kind"], np.int64)
    nq = len(c_off) - 1
    ms = clauses.get("q_min_should")
    ms = np.zeros(nq, np.int64) if ms is None else np.broadcast_to(np.asarray(ms, np.int64), (nq,))
    out = []
    for q in range(nq):
        ng = int(g_off[q + 1] - g_off[q])
        if ng == 0:
            out.append(None)
            continue
        kinds = kind[g_off[q]:g_off[q + 1]]
        per_seg = []
        for s, seg in enumerate(segs):
            held = np.zeros((ng, seg.n_docs), bool)
            for i in range(int(c_off[q]), int(c_off[q + 1])):
                t = int(terms[i, s])
                if t != NO_TERM:
                    held[group[i], postings(seg, t)] = True
            ok = np.ones(seg.n_docs, bool)
            for g in np.nonzero(kinds == MUST)[0]:
                ok &= held[g]
            for g in np.nonzero(kinds == MUST_NOT)[0]:
                ok &= ~held[g]
            ok &= held[kinds == SHOULD].sum(axis=0) >= int(ms[q])
            per_seg.append(ok)
        out.append(per_seg)
    return out


def accept_masks(segs, clauses, q_filter=None, filters=None):
    """the clause masks AND-ed with each query's own filter masks -> per query [mask or None per segment]"""
    out = []
    for q, cm in enumerate(clause_masks(segs, clauses)):
        per_seg = [None] * len(segs) if cm is None else list(cm)
        f = int(q_filter[q]) if q_filter is not None else -1
        if f >= 0:
            per_seg = [fm if pm is None else (pm if fm is None else (pm & np.asarray(fm, bool)))
                       for pm, fm in zip(per_seg, filters[f])]
        out.append(per_seg)
    return out


def reference(oracle, segs, q_offsets, q_terms, q_weights, k, clauses, q_filter=None, filters=None, strategy=None,
              **plans):
    """(doc, seg, score, count) of the bool batch"""
    masks = accept_masks(segs, clauses, q_filter, filters)
    nq = len(q_offsets) - 1
    return oracle.search_batch_filtered(segs, q_offsets, q_terms, q_weights, k, np.arange(nq), masks,
                                        strategy=oracle.BM25 if strategy is None else strategy, **plans)


def scored_docs(segs, q_offsets, q_terms, clauses):
    """per query: docs that hold a scored term and pass the clause mask (no tombstone, no filter: slg_stats)"""
    terms = np.asarray(q_terms, np.uint32).reshape(-1, len(segs))
    masks = clause_masks(segs, clauses)
    out = np.zeros(len(q_offsets) - 1, np.uint64)
    for q in range(len(out)):
        for s, seg in enumerate(segs):
            hit = np.zeros(seg.n_docs, bool)
            for i in range(int(q_offsets[q]), int(q_offsets[q + 1])):
                if int(terms[i, s]) != NO_TERM:
                    hit[postings(seg, int(terms[i, s]))] = True
            if masks[q] is not None:
                hit &= masks[q][s]
            out[q] += int(hit.sum())
    return out
