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


# ---- rerank reference (tests/test_rerank_bound.py, tests/test_gpu_rerank_widths.py) ---------------------
# A rerank case: `fields` = [dict(metric, dim, segs=[(offsets u32[n_docs], values f32[rows, dim]) or None
# per segment])]; a query `q` = dict(cf = field of each clause, qv = [f32[dim] per clause], alpha f32[nc],
# boost f32[nc] or None, seg / doc u32[n], bm f32[n]).  kind: "one" (rerank_kernel: one clause over
# field 0, no boost), "multi" (rerank_multi_kernel: clauses over field 0) or "fields"
# (rerank_fields_kernel).  A candidate has a vector in clause c iff its segment is < n_segs, has the
# field, and doc < that segment's n_docs with offsets[doc] != NO_VECTOR.
NO_VECTOR = 0xFFFFFFFF
F32_MAX = float(np.finfo(np.float32).max)
F32_MIN = -F32_MAX
U_F32 = 2.0 ** -24   # unit roundoff of f32
ETA_F32 = 2.0 ** -149  # absolute error of one f32 operation with a subnormal result


def _gamma(n):
    """gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, 3.1)."""
    return n * U_F32 / (1.0 - n * U_F32)


def _rnd(lo, hi):
    """[lo, hi] (float64 arrays) widened by the rounding of one f32 operation whose exact result lies in
    it: relative u, absolute ETA for subnormals; past F32_MAX the result may round to +-inf."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(invalid="ignore"):
        lo2 = np.where(np.isinf(lo), lo, lo - U_F32 * np.abs(lo) - ETA_F32)
        hi2 = np.where(np.isinf(hi), hi, hi + U_F32 * np.abs(hi) + ETA_F32)
    lo2 = np.where(lo2 < -F32_MAX, -np.inf, np.minimum(lo2, F32_MAX))
    hi2 = np.where(hi2 > F32_MAX, np.inf, np.maximum(hi2, -F32_MAX))
    return lo2, hi2


def _mul(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.stack([a[0] * b[0], a[0] * b[1], a[1] * b[0], a[1] * b[1]])
    return _rnd(np.fmin.reduce(c), np.fmax.reduce(c))


def _add(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return _rnd(a[0] + b[0], a[1] + b[1])


def rerank_row(field, seg, doc):
    """The row of (seg, doc) in a field, or None (no vector)."""
    segs = field["segs"]
    if seg >= len(segs) or segs[seg] is None:
        return None
    offs, vals = segs[seg]
    if doc >= len(offs) or offs[doc] == NO_VECTOR:
        return None
    return vals[offs[doc]]


def missing_score(metric):
    return -1.0 if metric == 0 else F32_MIN


def similarity_interval(metric, qv, rows, l2_identity=False):
    """[lo, hi] (float64 arrays over the rows) holding every f32 evaluation of metric_similarity(qv, row)
    (vectors/mod.rs:98-120), whatever the order of its sums.

    Cosine: an f32 inner product of n terms, in any summation order, differs from the exact sum of the
    exact products by at most gamma_n * sum |q_i x_i| (Higham 3.1: each product is rounded once, each
    term takes part in at most n - 1 rounded additions; adding the exact zeros of masked lanes rounds
    nothing), + n ETA for subnormal results.  A NaN sum scores 0 (vectors/mod.rs:112-116); an infinite
    one is exact.
    L2: sum (q_i - x_i)^2: each difference and square is rounded once more, so gamma_{n+2} * sum d_i^2
    (+ n ETA).  The matrix-core identity (l2_identity: rerank_multi_kernel with >= 3 L2 clauses and
    dim % 16 == 0) computes |q|^2 + |x|^2 - 2 q.x: three inner products of n terms, one addition and one
    subtraction, so gamma_{n+2} * (|q|^2 + |x|^2 + 2 sum |q_i x_i|); a near-duplicate pair it recomputes
    as the plain sum, so both bounds are added.  A sum past F32_MAX may be +inf (with nonnegative terms
    it is in every order once the exact sum is past it); the square root and the sign are one more
    rounding (relative u)."""
    q = np.asarray(qv, dtype=np.float64)
    x = np.asarray(rows, dtype=np.float64).reshape(-1, len(q))
    n = len(q)
    with np.errstate(all="ignore"):
        if metric == 0:
            p = x * q
            s = p.sum(axis=1)
            e = _gamma(n) * np.abs(p).sum(axis=1) + n * ETA_F32
            lo = np.where(s - e < -F32_MAX, -np.inf, s - e)
            hi = np.where(s + e > F32_MAX, np.inf, s + e)
            exact = np.isinf(s)
            lo, hi = np.where(exact, s, lo), np.where(exact, s, hi)
            nan = np.isnan(s)
            return np.where(nan, 0.0, lo), np.where(nan, 0.0, hi)
        d = q - x
        s = (d * d).sum(axis=1)
        assert not np.isnan(s).any(), "L2 NaN is out of scope"
        e = _gamma(n + 2) * s + n * ETA_F32
        if l2_identity:
            e = e + _gamma(n + 2) * ((q * q).sum() + (x * x).sum(axis=1) + 2 * np.abs(x * q).sum(axis=1))
        e = np.where(np.isinf(s), 0.0, e)
        slo, shi = np.maximum(s - e, 0.0), s + e
        shi = np.where(shi > F32_MAX, np.inf, shi)
        slo = np.where(slo > F32_MAX, np.inf, slo)
        return -np.sqrt(shi) * (1 + U_F32), -np.sqrt(slo) * (1 - U_F32)


def rerank_exact(fields, q, kind, l2_identity=False):
    """Per candidate, in float64: the interval of the blended score and of the reported vector score that
    every f32 evaluation of compute_hybrid_score (api/reader.rs:225-254) lies in.  The similarity carries
    the bound of similarity_interval; the boost, the blend alpha * bm + (1 - alpha) * vs, the clause sums
    (in clause order, as the reference and the kernels add them) and the division by the clause count
    each add one f32 rounding (_rnd) of the interval they produce.  -> (score_lo, score_hi, vec_lo,
    vec_hi), float64[n] each; an exact value has lo == hi."""
    n = len(q["doc"])
    nc = len(q["cf"])
    alpha = np.asarray(q["alpha"], np.float32).astype(np.float64).reshape(-1)
    boost = None if q.get("boost") is None else np.asarray(q["boost"], np.float32).astype(np.float64).reshape(-1)
    bm = np.asarray(q["bm"], np.float32).astype(np.float64)
    assert not np.isnan(bm).any(), "NaN bm25 values are checked bit for bit, not here"
    bsum = vsum = None
    has_any = np.zeros(n, bool)
    for c in range(nc):
        f = fields[q["cf"][c]]
        rows = [rerank_row(f, int(sg), int(d)) for sg, d in zip(q["seg"], q["doc"])]
        has = np.array([r is not None for r in rows], bool)
        has_any |= has
        miss = missing_score(f["metric"])
        vs = (np.full(n, miss), np.full(n, miss))
        if has.any():
            lo, hi = similarity_interval(f["metric"], q["qv"][c], np.stack([r for r in rows if r is not None]),
                                         l2_identity)
            if boost is not None:
                assert boost[c] > 0
                lo, hi = _mul((lo, hi), (boost[c], boost[c]))
            vs[0][has], vs[1][has] = lo, hi
            part = (np.where(has, vs[0], 0.0), np.where(has, vs[1], 0.0))
            vsum = part if vsum is None else _add(vsum, part)
        a = alpha[c]
        if a >= 1.0:
            bl = (bm, bm)
        elif a <= 0.0:
            bl = vs
        else:
            w = _rnd(1.0 - a, 1.0 - a)
            bl = _add(_mul((a, a), (bm, bm)), _mul(w, vs))
        bsum = bl if bsum is None else _add(bsum, bl)
    if kind != "one":
        lo, hi = bsum[0] / nc, bsum[1] / nc
        bsum = (lo, hi) if nc & (nc - 1) == 0 else _rnd(lo, hi)
    m0 = missing_score(fields[q["cf"][0]]["metric"])
    if vsum is None:
        vsum = (np.zeros(n), np.zeros(n))
    vlo, vhi = np.where(has_any, vsum[0], m0), np.where(has_any, vsum[1], m0)
    return np.asarray(bsum[0], np.float64), np.asarray(bsum[1], np.float64), vlo, vhi


def _f32_key(x):
    """f32::total_cmp key of an f32 (as numpy int64)."""
    b = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, b ^ 0x7FFFFFFF, b)


def check_rerank_result(fields, q, kind, k_out, got, l2_identity=False, what=""):
    """One query's kernel output got = (doc, seg, score, vec, count) (the query's row of each array) against
    the float64 intervals of rerank_exact: count = min(candidates, k_out); strict (score by total_cmp
    desc, seg, doc) order; every output a distinct real candidate; every score and vector score inside
    its interval; and no candidate left out whose interval lies above the k-th output (equal exact
    scores: the (seg, doc) order decides).  Near-ties need no absolute tolerance."""
    gd, gs, gsc, gv, gc = got
    n = len(q["doc"])
    slo, shi, vlo, vhi = rerank_exact(fields, q, kind, l2_identity)
    want_n = min(n, k_out)
    assert int(gc) == want_n, f"{what}: count {int(gc)} != {want_n}"
    gd, gs = np.asarray(gd[:want_n], np.int64), np.asarray(gs[:want_n], np.int64)
    gsc, gv = np.asarray(gsc[:want_n], np.float32), np.asarray(gv[:want_n], np.float32)
    key = _f32_key(gsc)
    for j in range(1, want_n):
        assert (key[j - 1], -gs[j - 1], -gd[j - 1]) > (key[j], -gs[j], -gd[j]), f"{what}: order at {j}"
    index = {}
    for i in range(n):
        index.setdefault((int(q["seg"][i]), int(q["doc"][i])), i)
    used = set()
    for j in range(want_n):
        i = index.get((int(gs[j]), int(gd[j])))
        assert i is not None, f"{what}: output {j} ({gs[j]}, {gd[j]}) is not a candidate"
        assert i not in used, f"{what}: output {j} ({gs[j]}, {gd[j]}) appears twice"
        used.add(i)
        s, v = float(gsc[j]), float(gv[j])
        assert slo[i] <= s <= shi[i], f"{what}: score of ({gs[j]}, {gd[j]}) {s!r} outside [{slo[i]!r}, {shi[i]!r}]"
        assert vlo[i] <= v <= vhi[i], f"{what}: vec score of ({gs[j]}, {gd[j]}) {v!r} outside [{vlo[i]!r}, {vhi[i]!r}]"
    if want_n == 0 or want_n == n:
        return
    ks, kseg, kdoc = float(gsc[-1]), int(gs[-1]), int(gd[-1])
    for i in range(n):
        if i in used:
            continue
        sk = (int(q["seg"][i]), int(q["doc"][i]))
        assert not (slo[i] > ks or (slo[i] == shi[i] == ks and sk < (kseg, kdoc))), \
            f"{what}: candidate {sk} (score >= {slo[i]!r}) left out below the k-th output {ks!r}"


def oracle_rerank_segments(oracle, fields, q, kind, k_out):
    """The oracle on candidates from several segments: each field's segments become one store with
    combined ids seg * N + doc (N above every segment's n_docs and every candidate doc, so the (seg, doc)
    order is kept); docs past their segment's n_docs, segments >= n_segs and segments without the field
    map to NO_VECTOR.  -> (doc, seg, score, vec) arrays of the top min(n, k_out)."""
    doc = np.asarray(q["doc"], np.int64)
    seg = np.asarray(q["seg"], np.int64)
    n_segs = len(fields[0]["segs"])
    N = 1 + max([int(doc.max()) if len(doc) else 0] +
                [len(s[0]) for f in fields for s in f["segs"] if s is not None])
    assert (max(n_segs, int(seg.max()) + 1 if len(seg) else 0)) * N < 2 ** 32
    comb = []
    for f in fields:
        offs = np.full(n_segs * N, NO_VECTOR, np.uint32)
        vals, base = [np.zeros((0, f["dim"]), np.float32)], 0
        for s, sd in enumerate(f["segs"]):
            if sd is None:
                continue
            o, v = sd
            offs[s * N:s * N + len(o)] = np.where(o == NO_VECTOR, NO_VECTOR, o.astype(np.int64) + base)
            vals.append(v)
            base += len(v)
        comb.append((f["metric"], offs, np.concatenate(vals)))
    cid = (seg * N + doc).astype(np.uint32)
    if kind == "one":
        m, offs, vals = comb[0]
        d, s_, v = oracle.rerank(m, offs, vals, q["qv"][0], float(np.float32(q["alpha"][0])), cid, q["bm"], k_out)
    elif kind == "multi":
        m, offs, vals = comb[0]
        d, s_, v = oracle.rerank_multi(m, offs, vals, np.stack(q["qv"]), q["alpha"], cid, q["bm"], k_out,
                                       boost=q.get("boost"))
    else:
        d, s_, v = oracle.rerank_fields(comb, list(q["cf"]), q["qv"], q["alpha"], cid, q["bm"], k_out,
                                        boost=q.get("boost"))
    d = np.asarray(d, np.int64)
    return (d % N).astype(np.uint32), (d // N).astype(np.uint32), s_, v
