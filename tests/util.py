"""Shared helpers for the parity tests (test infrastructure; may use the oracle)."""
from __future__ import annotations

import numpy as np


def random_segment(rng, n_docs, vocab, avg_len, k1=1.2, b=0.75, missing_len_frac=0.0,
                   zipf=True):
    """Small random one-field segment built directly as arrays (doc ids = 0..n_docs-1)."""
    from searchlite_amd.segment import Segment
    lens = rng.integers(max(1, avg_len // 2), avg_len * 2 + 1, size=n_docs)
    if zipf:
        p = 1.0 / np.arange(1, vocab + 1)
        p /= p.sum()
    else:
        p = np.full(vocab, 1.0 / vocab)
    post = [[] for _ in range(vocab)]
    for d in range(n_docs):
        toks = rng.choice(vocab, size=int(lens[d]), p=p)
        t, c = np.unique(toks, return_counts=True)
        for ti, ci in zip(t, c):
            post[int(ti)].append((d, int(ci)))
    offs = np.zeros(vocab + 1, dtype=np.uint64)
    docs, tfs = [], []
    for t in range(vocab):
        for d, c in post[t]:
            docs.append(d)
            tfs.append(c)
        offs[t + 1] = len(docs)
    dl = lens.astype(np.float32)
    if missing_len_frac > 0:
        miss = rng.random(n_docs) < missing_len_frac
        dl[miss] = 0.0
    avg = np.float32(np.float32(lens.sum()) / np.float32(n_docs))
    return Segment(n_docs=n_docs, term_offsets=offs, doc_ids=np.array(docs, dtype=np.uint32),
                   tfs=np.array(tfs, dtype=np.uint32), field_doc_len=[dl],
                   field_avgdl=np.array([avg], dtype=np.float32), docs=float(n_docs), k1=k1, b=b)


def random_multifield_segment(rng, n_docs, vocab, n_fields, avg_len, k1=0.9, b=0.4):
    """Random segment with n_fields text fields over the same vocabulary: term id = f*vocab + w
    (the `field:word` keys of index/postings.rs), per-field doc lengths / avgdl; some docs lack a
    field (length 0)."""
    from searchlite_amd.segment import Segment
    p = 1.0 / np.arange(1, vocab + 1)
    p /= p.sum()
    V = vocab * n_fields
    post = [[] for _ in range(V)]
    lens = np.zeros((n_fields, n_docs), dtype=np.float32)
    for f in range(n_fields):
        fl = max(1, avg_len // (f + 1))
        for d in range(n_docs):
            if rng.random() < 0.1:
                continue  # field missing in this doc
            n = int(rng.integers(max(1, fl // 2), fl * 2 + 1))
            toks = rng.choice(vocab, size=n, p=p)
            t, c = np.unique(toks, return_counts=True)
            for ti, ci in zip(t, c):
                post[f * vocab + int(ti)].append((d, int(ci)))
            lens[f, d] = n
    offs = np.zeros(V + 1, dtype=np.uint64)
    docs, tfs = [], []
    for t in range(V):
        for d, c in post[t]:
            docs.append(d)
            tfs.append(c)
        offs[t + 1] = len(docs)
    avg = np.array([np.float32(lens[f].sum()) / np.float32(n_docs) for f in range(n_fields)], dtype=np.float32)
    tfield = np.repeat(np.arange(n_fields, dtype=np.uint16), vocab)
    return Segment(n_docs=n_docs, term_offsets=offs, doc_ids=np.array(docs, dtype=np.uint32),
                   tfs=np.array(tfs, dtype=np.uint32), field_doc_len=[lens[f] for f in range(n_fields)],
                   field_avgdl=avg, docs=float(n_docs), k1=k1, b=b, term_field=tfield)


def skewed_segment(rng, n_docs, n_lists):
    """One-field segment built list by list (fast for millions of doc ids): list sizes from a few
    postings to ~n_docs/8, each either spread uniformly or packed into a narrow run of doc ids."""
    from searchlite_amd.segment import Segment
    offs, docs, tfs = [0], [], []
    for _ in range(n_lists):
        size = int(min(n_docs // 4, rng.choice([3, 40, 600, 5_000, 40_000, max(8, n_docs // 8)])))
        if rng.random() < 0.35:   # clustered: (almost) consecutive doc ids
            start = int(rng.integers(0, max(1, n_docs - size * 2)))
            d = start + np.unique(rng.integers(0, size * 2, size=size))
        else:
            d = np.unique(rng.integers(0, n_docs, size=size))
        d = d.astype(np.uint32)
        docs.append(d)
        tfs.append(rng.integers(1, 4, size=len(d)).astype(np.uint32))
        offs.append(offs[-1] + len(d))
    dl = rng.integers(5, 60, size=n_docs).astype(np.float32)
    return Segment(n_docs=n_docs, term_offsets=np.array(offs, dtype=np.uint64),
                   doc_ids=np.concatenate(docs), tfs=np.concatenate(tfs), field_doc_len=[dl],
                   field_avgdl=np.array([np.float32(dl.mean())], dtype=np.float32), docs=float(n_docs),
                   k1=1.2, b=0.75)


def random_queries(rng, nq, n_terms, vocab, n_segs=1, lo=0, weights=False):
    offs = (np.arange(nq + 1) * n_terms).astype(np.uint32)
    terms = np.empty((nq * n_terms, n_segs), dtype=np.uint32)
    for q in range(nq):
        t = rng.choice(np.arange(lo, vocab), size=n_terms, replace=False)
        for s in range(n_segs):
            terms[q * n_terms:(q + 1) * n_terms, s] = t
    w = (rng.random(nq * n_terms).astype(np.float32) * 2 + 0.25) if weights \
        else np.ones(nq * n_terms, dtype=np.float32)
    return offs, terms, w


def assert_same_hits(got, want, score_tol=0.0, what=""):
    """got/want = (doc[nq,k], seg[nq,k], score[nq,k], count[nq]).  Identical (seg, doc)
    sequence; scores bit-exact when score_tol == 0, else |d| <= score_tol."""
    gd, gs, gsc, gc = got
    wd, ws, wsc, wc = want
    assert gd.shape == wd.shape, f"{what}: shape {gd.shape} vs {wd.shape}"
    bad = []
    for q in range(len(wc)):
        n = int(wc[q])
        if int(gc[q]) != n:
            bad.append((q, "count", int(gc[q]), n))
            continue
        if not (np.array_equal(gd[q, :n], wd[q, :n]) and np.array_equal(gs[q, :n], ws[q, :n])):
            i = int(np.argmax((gd[q, :n] != wd[q, :n]) | (gs[q, :n] != ws[q, :n])))
            bad.append((q, f"doc@{i}", (int(gs[q, i]), int(gd[q, i]), float(gsc[q, i])),
                        (int(ws[q, i]), int(wd[q, i]), float(wsc[q, i]))))
            continue
        if score_tol == 0.0:
            if not np.array_equal(gsc[q, :n].view(np.uint32), wsc[q, :n].view(np.uint32)):
                i = int(np.argmax(gsc[q, :n].view(np.uint32) != wsc[q, :n].view(np.uint32)))
                bad.append((q, f"score@{i}", float(gsc[q, i]), float(wsc[q, i])))
        else:
            d = np.abs(gsc[q, :n].astype(np.float64) - wsc[q, :n].astype(np.float64))
            if d.size and d.max() > score_tol:
                bad.append((q, "score", float(d.max()), score_tol))
    assert not bad, f"{what}: {len(bad)} queries differ, first: {bad[:5]}"


GOLDEN = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden")


def load_golden(name):
    """-> (segments, npz) for a fixture written by tests/golden/make_golden.py."""
    import os
    from searchlite_amd.segment import Segment
    z = np.load(os.path.join(GOLDEN, name))

    def seg(prefix):
        nf = int(z[prefix + "n_fields"])
        lens = [z[prefix + f"doc_len{i}"] if (prefix + f"doc_len{i}") in z else None
                for i in range(nf)]
        return Segment(n_docs=int(z[prefix + "n_docs"]), term_offsets=z[prefix + "term_offsets"],
                       doc_ids=z[prefix + "doc_ids"], tfs=z[prefix + "tfs"], field_doc_len=lens,
                       field_avgdl=z[prefix + "field_avgdl"], docs=float(z[prefix + "docs"]),
                       k1=float(z[prefix + "k1"]), b=float(z[prefix + "b"]),
                       term_field=z[prefix + "term_field"] if (prefix + "term_field") in z else None)

    if "n_docs" in z:
        return [seg("")], z
    segs, i = [], 0
    while f"s{i}_n_docs" in z:
        segs.append(seg(f"s{i}_"))
        i += 1
    return segs, z


def golden_expected(z):
    return z["exp_doc"], z["exp_seg"], z["exp_score"], z["exp_count"]


# ---- top-k width matrix (tests/test_gpu_topk_widths.py, tests/test_plan.py) -------------------------
# Every scoring and merge kernel is compiled once per top-k register width (KREGS 1 / 2 / 4 / 8 / 16 for
# k <= 64 / 128 / 256 / 512 / more).  The families below each reach one scoring instantiation; the
# matrix runs each at k on both sides of every width boundary.
TOPK_WIDTH_KS = (1, 64, 65, 128, 129, 201, 256, 257, 512, 513, 1024, 1025)
TOPK_BOUNDARY_DFS = (64, 65, 128, 129, 256, 257, 1024, 1025)
TOPK_FAMILIES = ("F1", "F2", "F3", "F4", "F5", "F6", "F7", "F8", "F9")
# tuning variant (b): no threshold seed, so every posting enters the buffered top-k and it ranks many
# times per slice; one round per slice (rounds_per_slice pins it: max_rounds_per_slice only caps the
# slices that grow past the default), so the merge sees many slices per query
TOPK_ROUND_PER_SLICE = {"champions": 0, "rounds_per_slice": 1, "max_rounds_per_slice": 1}


def topk_variants(name):
    """-> {label: tuning overrides} the matrix runs family `name` under.  F6 (MaxScore-classified) keeps
    its champion table in variant (b): classification needs the threshold seed the table gives, and
    without it the batch would run unclassified (MODE 0, which F5 covers)."""
    b = dict(TOPK_ROUND_PER_SLICE)
    if name == "F6":
        del b["champions"]
    return {"a": {}, "b": b}


def _append_lists(seg, lists):
    """seg with extra terms appended after its vocabulary: lists = [(doc ids, tfs)]."""
    from searchlite_amd.segment import Segment
    offs = [np.asarray(seg.term_offsets, dtype=np.uint64)]
    docs, tfs = [seg.doc_ids], [seg.tfs]
    end = int(seg.term_offsets[-1])
    for d, t in lists:
        docs.append(np.asarray(d, dtype=np.uint32))
        tfs.append(np.asarray(t, dtype=np.uint32))
        end += len(d)
        offs.append(np.array([end], dtype=np.uint64))
    tf = None if seg.term_field is None else np.concatenate(
        [seg.term_field, np.zeros(len(lists), dtype=seg.term_field.dtype)])
    return Segment(n_docs=seg.n_docs, term_offsets=np.concatenate(offs), doc_ids=np.concatenate(docs),
                   tfs=np.concatenate(tfs), field_doc_len=seg.field_doc_len, field_avgdl=seg.field_avgdl,
                   docs=seg.docs, k1=seg.k1, b=seg.b, term_field=tf)


TOPK_FEW_DFS = (40, 100)   # live df of the one list queries 5 and 6 keep


def _make_few(terms, q, first, few_term):
    """Queries 5 and 6: the first term becomes crafted list few_term + (q - 5) of segment 0, every other
    term of the query is absent (the query keeps its leaves and plan)."""
    from searchlite_amd.segment import NO_TERM
    if q not in (5, 6):
        return
    for i in range(first, len(terms)):
        terms[i] = [NO_TERM, NO_TERM]
    terms[first] = [few_term + q - 5, NO_TERM]


def topk_family(name):
    """One batch of the top-k width matrix (fixed seeds; plain data, no device):
      F1 few-term, <= 4 lists (T = 3)             F6 many-term, pruning-classified (Wand, pruning 1)
      F2 few-term, 5..8 lists (T = 7, pruning 0)  F7 flat plans, uniform_plans 0 (many-term kernel)
      F3 flat Sum / DisMax plans, 2 fields x 2 words  F8 two-level plans
      F4 flat plans, 4 fields x 2 words           F9 a score tree of four internal levels
      F5 many-term, unclassified (T = 12, pruning 0)
    Two segments; every 7th doc deleted and made short (so deleted docs are among the top scorers);
    integer weights and short docs (scores tie exactly at the k-th place, the doc id decides); queries
    with no term at all, with far more matches than any k, and two with few: queries 5 and 6 keep one
    term, a crafted list of segment 0 with TOPK_FEW_DFS live docs (every other term absent).  F1 and F5
    add single-term queries on crafted lists of segment 0 whose live df is every TOPK_BOUNDARY_DFS value
    (count == k - 1, k, k + 1 at the width boundaries).  A doc filter (id 0) on every third query.
    -> dict(segs, offs, terms, w, plans (prepare() keywords), q_filter, masks (filter 0), tuning, strategy)."""
    from searchlite_amd.segment import NO_TERM
    fam = int(name[1:])
    rng = np.random.default_rng(5100 + fam)
    multifield = fam in (3, 4, 7, 8, 9)
    n_fields = 4 if fam == 4 else 3 if fam in (8, 9) else 2
    vocab = 12 if multifield else 40
    segs = []
    for s in range(2):
        n = 2600 + 700 * s
        if multifield:
            # (short text where queries span three or four fields: exact ties at the k-th place)
            sg = random_multifield_segment(rng, n, vocab, n_fields, 3 if n_fields >= 3 else 6)
        else:
            sg = random_segment(rng, n, vocab, 5)
        for dl in sg.field_doc_len:
            dl[::7] = np.where(dl[::7] > 0, 1.0, 0.0)   # deleted docs score high
        segs.append(sg)
    crafted = fam in (1, 5)
    # lists of live (not deleted) docs of segment 0 after its vocabulary: the boundary dfs (F1, F5), the few
    base = segs[0].n_terms
    live = np.array([d for d in range(segs[0].n_docs) if d % 7], dtype=np.uint32)
    lists = []
    for df in (TOPK_BOUNDARY_DFS if crafted else ()) + TOPK_FEW_DFS:
        d = np.sort(rng.choice(live, size=df, replace=False)).astype(np.uint32)
        lists.append((d, rng.integers(1, 3, size=df)))
    segs[0] = _append_lists(segs[0], lists)
    few_term = base + (len(TOPK_BOUNDARY_DFS) if crafted else 0)
    for sg in segs:
        sg.set_deleted(range(0, sg.n_docs, 7))
    nq = 28
    S, D, L = 0, 1, 2
    offs, terms, w = [0], [], []
    leaf, plan, tie, nl = [], [], [], []
    qlo, lg, qgo, gp, gt = [0], [], [0], [], []
    nk, nt, npar, qno = [], [], [], [0]
    T = {1: 3, 2: 7, 5: 12, 6: 12}.get(fam, 0)
    for q in range(nq):
        none = q == 3                                    # no term in any segment
        q_first = len(terms)
        if fam in (1, 2, 5, 6):
            if crafted and 8 <= q < 8 + len(TOPK_BOUNDARY_DFS):
                terms.append([base + q - 8, NO_TERM])
                w.append(np.float32(1.0))
            else:
                n_t = T if q % 4 else max(1, T // 2)     # ragged term counts
                for t in rng.choice(vocab, size=n_t, replace=False):
                    terms.append([NO_TERM if none else int(t)] * 2)
                    w.append(np.float32(1 + q % 2 * (int(t) % 2)))
            _make_few(terms, q, q_first, few_term)
            offs.append(len(terms))
            continue
        n_words = 2 if fam in (3, 4, 7) else 3
        words = rng.choice(vocab, size=n_words, replace=False)
        fields = n_fields if fam != 9 else 3
        for wi, wd in enumerate(words):
            for f in range(fields):
                t = f * vocab + int(wd)
                terms.append([NO_TERM if none else t] * 2)
                w.append(np.float32(1 + (f + wi) % 2))
                leaf.append(wi if fam != 9 else [0, 1, 1, 2, 3, 3, 4, 5, 5][wi * 3 + f])
        _make_few(terms, q, q_first, few_term)
        offs.append(len(terms))
        if fam in (3, 4, 7):     # query string (leaf per word, Sum) or best_fields-like DisMax
            plan.append(D if q % 2 else S)
            tie.append(0.5 if q % 2 else 0.0)
            nl.append(n_words)
        elif fam == 8:           # root DisMax over two Sum groups, or root Sum over a DisMax group + leaf
            plan.append(D if q % 2 else S)
            tie.append(0.25 if q % 2 else 0.0)
            nl.append(3)
            lg += [0, 0, 1] if q % 2 else [0, 1, 1]
            qlo.append(len(lg))
            gp += [S, S] if q % 2 else [D, S]
            gt += [0.0, 0.0] if q % 2 else [0.5, 0.0]
            qgo.append(len(gp))
        else:                    # four internal levels, a leaf hanging off every level (6 leaves)
            nk += [D, L, S, L, D, L, S, L, L, L]
            nt += [.25, 0, 0, 0, .75, 0, 0, 0, 0, 0]
            npar += [0, 0, 0, 2, 2, 4, 4, 6, 6, 0]
            qno.append(len(nk))
    plans = {}
    if fam in (3, 4, 7, 8):
        plans = dict(q_leaf=np.array(leaf, np.uint32), q_plan=np.array(plan, np.int32),
                     q_tie=np.array(tie, np.float32), q_nleaves=np.array(nl, np.uint32))
    if fam == 8:
        plans.update(q_leaf_offsets=np.array(qlo, np.uint32), leaf_group=np.array(lg, np.uint32),
                     q_group_offsets=np.array(qgo, np.uint32), group_plan=np.array(gp, np.int32),
                     group_tie=np.array(gt, np.float32))
    if fam == 9:
        plans = dict(q_leaf=np.array(leaf, np.uint32), q_node_offsets=np.array(qno, np.uint32),
                     node_kind=np.array(nk, np.int32), node_tie=np.array(nt, np.float32),
                     node_parent=np.array(npar, np.uint32))
    q_filter = np.array([0 if q % 3 == 1 and not (crafted and 8 <= q < 16) else -1 for q in range(nq)],
                        dtype=np.int32)
    masks = [rng.random(sg.n_docs) < 0.6 for sg in segs]
    tuning = {2: {"pruning": 0}, 5: {"pruning": 0}, 6: {"pruning": 1, "block_max": 1},
              7: {"uniform_plans": 0}}.get(fam, {})
    return dict(segs=segs, offs=np.array(offs, np.uint32), terms=np.array(terms, np.uint32),
                w=np.array(w, np.float32), plans=plans, q_filter=q_filter, masks=masks, tuning=tuning,
                strategy=1)   # Wand (pruning-classified where pruning allows it)
