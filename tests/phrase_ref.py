"""Numpy / Python restatement of the phrase matcher (QueryEvaluator::phrase_matches, api/reader.rs:1584-1597;
build_phrase_runtimes, :1686-1720; matches_phrase, query/phrase.rs:4-48) in the flat form of
slg_batch_prepare_phrase, over the oracle and beside tests/bool_ref.py.

THE DEFINITION (restated from include/searchlite_gpu.h; the tests are bit-exact against it):
  * A phrase group has a slop and zero or more variants; a variant is an ordered row of n >= 1 terms.  In segment
    s a variant is dropped if any of its terms is NO_TERM there or has df 0.  A group holds a doc iff any
    surviving variant matches it; a group with no surviving variant holds nothing.  A segment without positions
    has an empty position list for every posting.
  * A variant matches a doc iff every term has a posting of the doc with at least one position (also for
    n = 1), and, for n >= 2, positions p0 < p1 < ... < p(n-1) exist, p_i from term i's list of the doc, with
    sum(p_i - p_(i-1) - 1) <= slop — i.e. p(n-1) - p0 <= slop + n - 1 over strictly increasing chains.  The same
    list may appear twice; strictness then demands two different positions.
  * Phrase groups are numbered after the query's term groups and enter the clause formula of a bool batch: a doc
    passes iff every MUST group (term or phrase) holds it, no MUST_NOT group does, and at least min_should SHOULD
    groups (term or phrase) do.

  1. matches(): the definition by EXHAUSTIVE search over all strictly increasing chains — deliberately not the
     greedy the kernel runs; matches_greedy(): that greedy, checked against matches() in tests/test_phrase_ref.py.
  2. clause_masks(): per (query, segment) one pass mask over the segment's docs, over term groups (a
     bool_ref.clauses_of dict or None) and phrase groups; None for a query without any group.
  3. reference(): oracle.search_batch_filtered with that mask as the query's filter, as bool_ref.reference.
  4. scored_docs(): the docs of the scored lists the clause mask passes.
phrases_of() builds the spec's arrays; segment_from_tokens() builds a segment whose postings, tfs and positions
come from the same token sequences."""
import numpy as np

from tests import bool_ref as B

MUST, SHOULD, MUST_NOT = B.MUST, B.SHOULD, B.MUST_NOT
NO_TERM = B.NO_TERM


def matches(lists, slop):
    """lists: per phrase position the positions (non-decreasing) of that term in the doc -> bool"""
    lists = [[int(p) for p in l] for l in lists]
    if any(len(l) == 0 for l in lists):
        return False
    n = len(lists)
    if n == 1:
        return True

    def chains(i, prev, first):  # every strictly increasing chain, no pruning
        if i == n:
            return prev - first <= slop + n - 1
        return any(chains(i + 1, p, first) for p in lists[i] if p > prev)

    return any(chains(1, p0, p0) for p0 in lists[0])


def matches_greedy(lists, slop):
    """the kernel's chain test: per start the smallest position above the previous pick in every following list,
    cursors that only move forward, stop when a list has nothing above the previous pick"""
    lists = [[int(p) for p in l] for l in lists]
    if any(len(l) == 0 for l in lists):
        return False
    n = len(lists)
    if n == 1:
        return True
    cur = [0] * n
    while cur[0] < len(lists[0]):
        p0 = prev = lists[0][cur[0]]
        for i in range(1, n):
            while cur[i] < len(lists[i]) and lists[i][cur[i]] <= prev:
                cur[i] += 1
            if cur[i] == len(lists[i]):
                return False
            prev = lists[i][cur[i]]
        if prev - p0 <= slop + n - 1:
            return True
        cur[0] += 1
    return False


def phrases_of(queries, n_segs):
    """queries: per query (phrases, min_should), phrases = [(kind, slop, [variant, ...])], variant = [term, ...],
    term = one id for every segment or a sequence of one id per segment -> the dict of search_batch_phrase"""
    p_offsets, p_kind, p_slop, v_offsets, t_offsets, t_terms, ms = [0], [], [], [0], [0], [], []
    for phrases, min_should in queries:
        for kind, slop, variants in phrases:
            p_kind.append(kind)
            p_slop.append(slop)
            for var in variants:
                for t in var:
                    t_terms.append([t] * n_segs if np.ndim(t) == 0 else list(t))
                t_offsets.append(len(t_terms))
            v_offsets.append(len(t_offsets) - 1)
        p_offsets.append(len(p_kind))
        ms.append(min_should)
    return dict(p_offsets=np.array(p_offsets, np.uint32), p_kind=np.array(p_kind, np.int32),
                p_slop=np.array(p_slop, np.uint32), v_offsets=np.array(v_offsets, np.uint32),
                t_offsets=np.array(t_offsets, np.uint32), t_terms=np.array(t_terms, np.uint32).reshape(-1, n_segs),
                q_min_should=np.array(ms, np.uint32))


def doc_positions(seg, term, doc):
    """the position list of the term's posting of the doc, or None without such a posting"""
    a, b = int(seg.term_offsets[term]), int(seg.term_offsets[term + 1])
    i = a + int(np.searchsorted(seg.doc_ids[a:b], doc))
    if i >= b or int(seg.doc_ids[i]) != doc:
        return None
    if seg.pos_offsets is None:
        return []
    return seg.positions[int(seg.pos_offsets[i]):int(seg.pos_offsets[i + 1])].tolist()


def phrase_holds(seg, s, slop, variants, t_terms):
    """bool[n_docs]: the docs of segment s (ordinal) the phrase group holds; variants: [(first row, end row)]"""
    held = np.zeros(seg.n_docs, bool)
    for t0, t1 in variants:
        ids = [int(t_terms[i, s]) for i in range(t0, t1)]
        if any(t == NO_TERM or seg.df(t) == 0 for t in ids):
            continue  # dropped in this segment
        docs = B.postings(seg, ids[0])
        for t in ids[1:]:
            docs = np.intersect1d(docs, B.postings(seg, t))
        for d in docs:
            if not held[d] and matches([doc_positions(seg, t, int(d)) for t in ids], slop):
                held[d] = True
    return held


def clause_masks(segs, clauses, phrases):
    """-> per query None (no group: untouched) or [one bool mask per segment]"""
    p_off = np.asarray(phrases["p_offsets"], np.int64)
    nq = len(p_off) - 1
    t_terms = np.asarray(phrases["t_terms"], np.uint32).reshape(-1, len(segs))
    v_off, t_off = np.asarray(phrases["v_offsets"], np.int64), np.asarray(phrases["t_offsets"], np.int64)
    ms = phrases.get("q_min_should")
    ms = np.zeros(nq, np.int64) if ms is None else np.broadcast_to(np.asarray(ms, np.int64), (nq,))
    if clauses is not None:
        assert clauses.get("q_min_should") is None, "the phrase spec states min_should"
        c_off, g_off = np.asarray(clauses["c_offsets"], np.int64), np.asarray(clauses["g_offsets"], np.int64)
        c_terms = np.asarray(clauses["c_terms"], np.uint32).reshape(-1, len(segs))
        c_group, g_kind = np.asarray(clauses["c_group"], np.int64), np.asarray(clauses["g_kind"], np.int64)
    out = []
    for q in range(nq):
        n_tg = int(g_off[q + 1] - g_off[q]) if clauses is not None else 0
        n_pg = int(p_off[q + 1] - p_off[q])
        if n_tg + n_pg == 0:
            out.append(None)
            continue
        kinds = np.concatenate([g_kind[g_off[q]:g_off[q + 1]] if n_tg else np.zeros(0, np.int64),
                                np.asarray(phrases["p_kind"], np.int64)[p_off[q]:p_off[q + 1]]])
        per_seg = []
        for s, seg in enumerate(segs):
            held = np.zeros((n_tg + n_pg, seg.n_docs), bool)
            if n_tg:
                for i in range(int(c_off[q]), int(c_off[q + 1])):
                    if int(c_terms[i, s]) != NO_TERM:
                        held[c_group[i], B.postings(seg, int(c_terms[i, s]))] = True
            for pi in range(n_pg):  # numbered after the term groups
                p = int(p_off[q]) + pi
                variants = [(int(t_off[v]), int(t_off[v + 1])) for v in range(int(v_off[p]), int(v_off[p + 1]))]
                held[n_tg + pi] = phrase_holds(seg, s, int(phrases["p_slop"][p]), variants, t_terms)
            ok = np.ones(seg.n_docs, bool)
            for g in np.nonzero(kinds == MUST)[0]:
                ok &= held[g]
            for g in np.nonzero(kinds == MUST_NOT)[0]:
                ok &= ~held[g]
            ok &= held[kinds == SHOULD].sum(axis=0) >= int(ms[q])
            per_seg.append(ok)
        out.append(per_seg)
    return out


def accept_masks(segs, clauses, phrases, q_filter=None, filters=None):
    """the clause masks AND-ed with each query's own filter masks -> per query [mask or None per segment]"""
    out = []
    for q, cm in enumerate(clause_masks(segs, clauses, phrases)):
        per_seg = [None] * len(segs) if cm is None else list(cm)
        f = int(q_filter[q]) if q_filter is not None else -1
        if f >= 0:
            per_seg = [fm if pm is None else (pm if fm is None else (pm & np.asarray(fm, bool)))
                       for pm, fm in zip(per_seg, filters[f])]
        out.append(per_seg)
    return out


def reference(oracle, segs, q_offsets, q_terms, q_weights, k, phrases, clauses=None, q_filter=None, filters=None,
              strategy=None, **plans):
    """(doc, seg, score, count) of the phrase batch"""
    masks = accept_masks(segs, clauses, phrases, q_filter, filters)
    nq = len(q_offsets) - 1
    return oracle.search_batch_filtered(segs, q_offsets, q_terms, q_weights, k, np.arange(nq), masks,
                                        strategy=oracle.BM25 if strategy is None else strategy, **plans)


def scored_docs(segs, q_offsets, q_terms, phrases, clauses=None):
    """per query: docs that hold a scored term and pass the clause mask (no tombstone, no filter: slg_stats)"""
    terms = np.asarray(q_terms, np.uint32).reshape(-1, len(segs))
    masks = clause_masks(segs, clauses, phrases)
    out = np.zeros(len(q_offsets) - 1, np.uint64)
    for q in range(len(out)):
        for s, seg in enumerate(segs):
            hit = np.zeros(seg.n_docs, bool)
            for i in range(int(q_offsets[q]), int(q_offsets[q + 1])):
                if int(terms[i, s]) != NO_TERM:
                    hit[B.postings(seg, int(terms[i, s]))] = True
            if masks[q] is not None:
                hit &= masks[q][s]
            out[q] += int(hit.sum())
    return out


def segment_from_tokens(docs, vocab, extra_postings=None, k1=1.2, b=0.75):
    """A one-field segment from token sequences: docs = per doc the list of term ids in text order (position i =
    index i), so doc ids, tfs and positions agree.  extra_postings: {term: [doc, ...]} postings WITHOUT a
    position (tf 1, an empty position list), merged into the term's list."""
    from searchlite_amd.segment import Segment
    post = [dict() for _ in range(vocab)]
    for d, toks in enumerate(docs):
        for i, t in enumerate(toks):
            post[int(t)].setdefault(d, []).append(i)
    for t, ds in (extra_postings or {}).items():
        for d in ds:
            assert d not in post[t]
            post[t][d] = []
    offs = np.zeros(vocab + 1, np.uint64)
    doc_ids, tfs, pos, pos_offs = [], [], [], [0]
    for t in range(vocab):
        for d in sorted(post[t]):
            doc_ids.append(d)
            tfs.append(max(len(post[t][d]), 1))
            pos.extend(post[t][d])
            pos_offs.append(len(pos))
        offs[t + 1] = len(doc_ids)
    lens = np.array([max(len(x), 1) for x in docs], np.float32)
    avg = np.float32(np.float32(lens.sum()) / np.float32(len(docs)))
    return Segment(n_docs=len(docs), term_offsets=offs, doc_ids=np.array(doc_ids, np.uint32),
                   tfs=np.array(tfs, np.uint32), field_doc_len=[lens], field_avgdl=np.array([avg], np.float32),
                   docs=float(len(docs)), k1=k1, b=b, pos_offsets=np.array(pos_offs, np.uint64),
                   positions=np.array(pos, np.uint32))
