"""Phrase queries on the device (slg_index_set_positions, slg_batch_prepare_phrase, slg_search_batch_phrase)
through the C ABI against tests/phrase_ref.py.  Tolerance 0: docs, segments, scores (bit patterns), counts,
scored_docs and matched counts are identical to the reference; rows past the count are zero.  Every corpus is built
from token sequences, so postings, tfs and positions agree."""
import copy

import numpy as np
import pytest

from tests import bool_ref as B
from tests import phrase_ref as P
from tests.test_gpu_bool import csr, dead_bitmap, same
from tests.test_gpu_sort import check as check_sorted, expected_rows

pytestmark = pytest.mark.gpu
F32 = np.float32
NO_TERM = 0xFFFFFFFF
MUST, SHOULD, MUST_NOT = P.MUST, P.SHOULD, P.MUST_NOT
KS = (1, 11, 257, 1025)


def specs_of(queries, n_segs):
    """queries: per query (term groups as bool_ref.clauses_of takes them, phrases as phrase_ref.phrases_of takes
    them, min_should) -> (clauses or None, phrases)"""
    cl = None
    if any(tg for tg, _, _ in queries):
        cl = B.clauses_of([(tg, 0) for tg, _, _ in queries], n_segs)
        del cl["q_min_should"]  # the phrase spec states it
    return cl, P.phrases_of([(ph, ms) for _, ph, ms in queries], n_segs)


class World:
    def __init__(self, sa, oracle, segs, positions_for=None, **tuning):
        self.oracle, self.segs, self.n_segs = oracle, segs, len(segs)
        self.ix = sa.GpuIndex(segs, **tuning)
        for s, seg in enumerate(segs):
            if positions_for is None or s in positions_for:
                self.ix.set_positions(s, seg.pos_offsets, seg.positions)
            else:
                seg.pos_offsets = seg.positions = None  # (the reference sees what the device sees)

    def check(self, qs, queries, k, what, **kw):
        cl, ph = specs_of(queries, self.n_segs)
        flt = {n: kw.pop(n) for n in ("q_filter", "filters") if n in kw}
        got = self.ix.search_batch_phrase(*qs, k, ph, clauses=cl, want_stats=True, q_filter=flt.get("q_filter"), **kw)
        want = P.reference(self.oracle, self.segs, *qs, k, ph, clauses=cl, **flt, **kw)
        same(got, want, what)
        sd = P.scored_docs(self.segs, qs[0], qs[1], ph, cl)
        got_sd = [int(got[4][q].scored_docs) for q in range(len(sd))]
        assert got_sd == sd.tolist(), f"{what}: scored_docs {got_sd} != {sd.tolist()}"
        assert [int(got[4][q].candidates_examined) for q in range(len(sd))] == sd.tolist()
        return got


# ---- world T: one segment of 4400 docs; every doc starts with ALL, then its crafted tokens, then filler ----
N_T = 4400
FILL = 8                      # filler vocabulary 0 .. 7
ALL, X, Y = 8, 9, 10          # ALL: every doc; X / Y: the position-count docs
REP = {20: 1, 21: 2, 22: 63, 23: 64, 24: 65, 25: 300}  # doc -> occurrences of X in front of one Y
NOPOS_DOC = 26                # holds a posting of X and of Y WITHOUT positions


@pytest.fixture(scope="module")
def T(oracle):
    import searchlite_amd as sa
    rng = np.random.default_rng(23)
    n = N_T
    ends = np.array([0, 3000, n - 1])

    def with_ends(df, pool=None):
        pool = np.setdiff1d(np.arange(1, n - 1) if pool is None else pool, ends)
        return np.sort(np.concatenate([ends, rng.choice(pool, size=df - len(ends), replace=False)]))

    c129 = with_ends(129)
    others = np.setdiff1d(np.arange(n), c129)
    lists = {"one": np.array([3000]), "d64": with_ends(64), "d65": with_ends(65), "d4096": with_ends(4096),
             "c1": np.array([3000]), "c63": with_ends(63), "c64": with_ends(64), "c65": with_ends(65), "c129": c129}
    for m in (63, 64, 65):  # m docs of c129 (its first and last among them) and 300 docs outside it
        lists[f"k{m}"] = np.sort(np.concatenate([with_ends(m, pool=c129), rng.choice(others, 300, replace=False)]))
    lists["none"] = np.sort(rng.choice(others, 500, replace=False))
    tok = {name: 11 + i for i, name in enumerate(lists)}
    LAST = 11 + len(lists)  # the last term of the vocabulary: its last posting is the last of the segment's arrays
    member = [[] for _ in range(n)]
    for name, ds in lists.items():
        for d in ds:
            member[int(d)].append(tok[name])
    docs = []
    for d in range(n):
        toks = [ALL] + member[d] + rng.integers(0, FILL, size=int(rng.integers(1, 6))).tolist()
        if d in REP:
            toks += [X] * REP[d] + [Y]
        if d in (40, n - 1):
            toks += [ALL, LAST]
        docs.append(toks)
    seg = P.segment_from_tokens(docs, LAST + 1, extra_postings={X: [NOPOS_DOC], Y: [NOPOS_DOC]})
    assert int(seg.doc_ids[-1]) == n - 1 and int(seg.pos_offsets[-1]) == len(seg.positions)
    W = World(sa, oracle, [seg])
    W.tok, W.lists, W.LAST, W.rng = tok, lists, LAST, rng
    yield W
    W.ix.close()


def one_term_queries(terms):
    return csr([[(t, 1.0 + 0.25 * i)] for i, t in enumerate(terms)], 1)


def must(*variants, slop=0, kind=MUST):
    return (kind, slop, [list(v) for v in variants])


def test_position_counts_and_the_last_posting(T):
    """postings with 0, 1, 2, 63, 64, 65 and 300 positions: the chain test walks X's list to its last start; the
    posting without positions fails also the one-term phrase; the final offset of the segment is read"""
    W = T
    phrases = [must([X, Y]), must([Y, X]), must([X]), must([X, X]), must([X, Y], slop=63), must([ALL, T.LAST]),
               must([T.LAST]), must([X, X, Y], slop=0), must([X, X, X], slop=61)]
    qs = one_term_queries([ALL] * len(phrases))
    queries = [([], [p], 0) for p in phrases]
    cl, ph = specs_of(queries, 1)
    left = P.scored_docs(W.segs, qs[0], qs[1], ph, cl).tolist()
    # "X Y": all six; "Y X": none; X alone: six (not the posting without positions); "X X": five; slop 63: the
    # same six; "ALL LAST" and LAST: docs 40 and the last; "X X Y": five; "X X X" within a span of 63: 4 (>= 3 X)
    assert left == [6, 0, 6, 5, 6, 2, 2, 5, 4]
    got = W.check(qs, queries, 11, "position counts")
    assert set(got[0][0, :6].tolist()) == set(REP) and N_T - 1 in got[0][5, :2].tolist()
    assert NOPOS_DOC not in got[0][2, :got[3][2]].tolist()


def test_list_edges(T):
    """phrase lists of df 1, 64, 65 and 4096 whose first and last postings (docs 0 and 4399; 3000 for df 1) are
    candidates: found under MUST (kept) and under MUST_NOT (dropped)"""
    W, tok = T, T.tok
    names = ["one", "d64", "d65", "d4096"]
    qs = one_term_queries([tok["c129"]] * (2 * len(names)))
    queries = [([], [must([tok[nm]])], 0) for nm in names] + [([], [must([tok[nm]], kind=MUST_NOT)], 0) for nm in names]
    got = W.check(qs, queries, 257, "list edges")
    for i, nm in enumerate(names):
        kept = set(got[0][i, :got[3][i]].tolist())
        dropped = set(got[0][len(names) + i, :got[3][len(names) + i]].tolist())
        for d in ((3000,) if nm == "one" else (0, 3000, N_T - 1)):
            assert d in kept and d not in dropped, (nm, d)
        assert kept | dropped == set(W.lists["c129"].tolist()) and not (kept & dropped)


def test_chunk_edges_of_the_compaction(T):
    """regions of 1, 63, 64, 65, 129 candidates (one slice each) left with 0, 1, 63, 64, 65, 129 survivors"""
    W, tok = T, T.tok
    scored = ["c1", "c63", "c64", "c65", "c129", "c129", "c129", "c129", "c129", "c129", "c129"]
    qs = one_term_queries([tok[nm] for nm in scored])
    queries = [([], [must([ALL])], 0), ([], [must([ALL])], 0), ([], [must([tok["none"]], kind=SHOULD), must([ALL], kind=SHOULD)], 1),
               ([], [must([ALL], kind=SHOULD)], 1), ([], [must([ALL])], 0), ([], [must([ALL], kind=MUST_NOT)], 0),
               ([], [must([tok["one"]])], 0), ([], [must([tok["k63"]])], 0), ([], [must([tok["k64"]], kind=SHOULD)], 1),
               ([], [must([ALL, tok["k65"]], slop=20)], 0), ([], [must([tok["none"]])], 0)]
    cl, ph = specs_of(queries, 1)
    left = P.scored_docs(W.segs, qs[0], qs[1], ph, cl).tolist()
    assert [len(W.lists[nm]) for nm in scored] == [1, 63, 64, 65, 129, 129, 129, 129, 129, 129, 129]
    assert left == [1, 63, 64, 65, 129, 0, 1, 63, 64, 65, 0]
    b = W.ix.prepare(*qs, 11, phrases=ph)
    assert b.info()["n_slices"] == len(scored)  # one slice per query: a region is a slice
    b.close()
    for k in (11, 257):
        got = W.check(qs, queries, k, f"chunk edges k={k}")
        assert got[3].tolist() == [min(x, k) for x in left]


def test_many_slices(T):
    """4400 candidates over several slices: all rejected, none rejected, a sparse and a dense phrase"""
    W, tok = T, T.tok
    qs = csr([[(ALL, 1.0), (int(t), 0.5)] for t in (3, 5, 7, 1)], 1)
    queries = [([], [must([ALL], kind=MUST_NOT)], 0), ([], [must([ALL])], 0), ([], [must([ALL, 2], slop=3)], 0),
               ([(MUST_NOT, [tok["d4096"]])], [must([1, 2], [2, 1], kind=SHOULD), must([ALL, tok["d64"]], kind=SHOULD, slop=9)], 1)]
    b = W.ix.prepare(*qs, 11, phrases=specs_of(queries, 1)[1], clauses=specs_of(queries, 1)[0])
    assert b.info()["n_slices"] > 4
    b.close()
    for k in KS:
        got = W.check(qs, queries, k, f"many slices k={k}")
        assert got[3].tolist()[:2] == [0, k] and got[3][2] > 0 and got[3][3] > 0


def test_term_groups_alone_equal_the_bool_batch(T):
    """A clause table of term groups only, once as a bool batch and once as a phrase batch whose spec gives no
    query a phrase (q_min_should moves to it): the phrase kernel's term pass may then accept early, as the bool
    kernel's does, and both batches return the same rows, counts, scored_docs and matched counts, bit for bit.
    Rows of 1, 4, 5 and 9 clause terms (a full step, a step with one live list, three steps) over lists of df 0
    (an absent term), 1, 63, 64, 65 and 129, against regions of 1, 63, 64, 65 and 129 candidates."""
    W, tok = T, T.tok
    mix = [(MUST, [ALL, tok["c1"]]), (MUST, [tok["c129"], tok["c65"]]), (MUST_NOT, [tok["k64"]]),  # MUST_NOT: the 5th term
           (SHOULD, [tok["c63"]]), (SHOULD, [tok["c64"], NO_TERM]), (SHOULD, [tok["k65"]])]
    table = [("c129", [(MUST, [tok["k63"]])], 0),                                                  # MUST only, 1 term
             ("c63", [(MUST_NOT, [tok["c1"], NO_TERM]), (MUST_NOT, [tok["c64"], tok["none"]])], 0),  # MUST_NOT only, 4
             ("c64", [(SHOULD, [tok["c63"], tok["c65"]]), (SHOULD, [tok["c129"]]), (SHOULD, [ALL, NO_TERM])], 2),  # 5
             ("c65", mix, 1), ("c129", mix, 1),                                                    # 9 terms
             ("c1", [(MUST, [tok["c1"]])], 0), ("c129", [(SHOULD, [tok["k65"]]), (SHOULD, [NO_TERM])], 2)]
    assert [sum(len(t) for _, t in groups) for _, groups, _ in table] == [1, 4, 5, 9, 9, 1, 2]
    qs = one_term_queries([tok[nm] for nm, _, _ in table])
    as_bool = B.clauses_of([(groups, ms) for _, groups, ms in table], 1)
    cl, ph = specs_of([(groups, [], ms) for _, groups, ms in table], 1)
    assert "q_min_should" not in cl and ph["p_offsets"].tolist() == [0] * (len(table) + 1)
    left = B.scored_docs(W.segs, qs[0], qs[1], as_bool).tolist()
    assert left[0] == 63 and left[5] == 1 and left[6] == 0 and 0 < left[1] < 63 and 0 < left[2] < 64
    score_order = [("_score", "desc")]  # (a sort spec: the batch has matched counts)
    for k in (1, 11):
        for sort in (None, score_order):
            what = f"term groups alone k={k} sort={sort}"
            a = W.ix.search_batch_bool(*qs, k, as_bool, sort=sort, want_stats=True)
            b = W.ix.search_batch_phrase(*qs, k, ph, clauses=cl, sort=sort, want_stats=True)
            same(b[:4], a[:4], what)
            for q in range(len(table)):
                assert int(b[4][q].scored_docs) == int(a[4][q].scored_docs) == left[q], f"{what}: scored_docs of query {q}"
                assert int(b[4][q].candidates_examined) == int(a[4][q].candidates_examined)
            assert a[3].tolist() == [min(x, k) for x in left], what
            if sort is not None:
                assert np.array_equal(np.asarray(b[5]), np.asarray(a[5])) and np.asarray(a[5]).tolist() == left, what


# ---- world S: crafted docs for the phrase shapes; every doc starts with term 0 (the scored term) ----
S_DOCS = [
    [0, 1, 2, 3, 4, 5, 6, 7, 8],          # 0: the 8-term phrase 1..8
    [0, 1, 2, 3, 4, 5, 6, 8, 7],          # 1: its last two swapped
    [0, 1, 9, 2, 3, 4, 5, 6, 7, 9, 8],    # 2: the 8 terms with two gaps: slop 2 exactly
    [0, 1],                               # 3: one occurrence of 1
    [0, 1, 9, 1],                         # 4: two occurrences, one gap
    [0, 1, 1],                            # 5: two adjacent occurrences
    [0, 1, 9, 9, 2, 9, 9, 9, 3],          # 6: "1 2 3" needs slop 2 + 3 = 5
    [0, 1, 9, 9, 9, 9, 9, 9, 9, 9, 1, 2], # 7: the first start of 1 fails at slop 0, the later one succeeds
    [0, 2, 2, 1, 2],                      # 8: "1 2" must skip the 2s in front of the 1
    [0, 2, 2, 1],                         # 9: ... and finds none
    [0, 3, 2, 1],                         # 10: reversed
    [0, 9, 9, 9],                         # 11
    [0, 1, 2, 9, 1, 9, 2, 9, 9, 1, 9, 9, 2],  # 12: gaps 0, 1, 2 between 1 and 2
]


@pytest.fixture(scope="module")
def S(oracle):
    import searchlite_amd as sa
    W = World(sa, oracle, [P.segment_from_tokens(S_DOCS, 10)])
    yield W
    W.ix.close()


def test_phrase_shapes(S):
    """phrases of 1, 2, 3 and 8 terms; "1 1" on docs with one and with two occurrences; slop 0, exactly enough and
    one short; the later-start case and the skip case"""
    eight = list(range(1, 9))
    cases = [(must([1]), [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12]), (must([1, 2]), [0, 1, 7, 8, 12]),
             (must([1, 2, 3]), [0, 1]), (must(eight), [0]), (must(eight, slop=1), [0]), (must(eight, slop=2), [0, 2]),
             (must([1, 1]), [5]), (must([1, 1], slop=1), [4, 5]), (must([1, 1], slop=99), [4, 5, 7, 12]),
             (must([1, 2, 3], slop=4), [0, 1, 2]), (must([1, 2, 3], slop=5), [0, 1, 2, 6]),
             (must([2, 1]), [8, 9, 10]), (must([3, 2, 1]), [10]), (must([9, 1, 2], slop=1), [7, 12]),
             (must([1, 2], kind=MUST_NOT), [2, 3, 4, 5, 6, 9, 10, 11]), (must([2], [9, 9, 9]), [0, 1, 2, 6, 7, 8, 9, 10, 11, 12])]
    qs = one_term_queries([0] * len(cases))
    queries = [([], [p], 0) for p, _ in cases]
    cl, ph = specs_of(queries, 1)
    masks = P.clause_masks(S.segs, cl, ph)
    for (p, want), m in zip(cases, masks):
        assert m[0].nonzero()[0].tolist() == want, p  # on the CPU first: hand-derived
    got = S.check(qs, queries, 33, "phrase shapes")
    for i, (_, want) in enumerate(cases):
        assert sorted(got[0][i, :got[3][i]].tolist()) == want


# ---- world A: two segments of random token docs over a vocabulary of 12, tombstones in both ----
def token_docs(rng, n, vocab=12):
    p = 1.0 / np.arange(1, vocab + 1)
    return [rng.choice(vocab, size=int(rng.integers(1, 13)), p=p / p.sum()).tolist() for _ in range(n)]


def world_a(oracle, positions_for=None, seed=17, **tuning):
    import searchlite_amd as sa
    rng = np.random.default_rng(seed)
    segs = [P.segment_from_tokens(token_docs(rng, 300), 12), P.segment_from_tokens(token_docs(rng, 200), 12)]
    segs[0].deleted = dead_bitmap(rng, 300, 0.1)
    segs[1].deleted = dead_bitmap(rng, 200, 0.15)
    segs[0].docs, segs[1].docs = [float(s.n_docs - np.unpackbits(s.deleted, bitorder="little")[:s.n_docs].sum()) for s in segs]
    W = World(sa, oracle, segs, positions_for, **tuning)
    W.rng = rng
    # 16 three-term queries; term 0 (in most docs) is scored by every one, so the candidates are many
    W.qs = csr([[(0, 1.0), (1 + q % 5, 0.75), (6 + q % 6, 1.5)] for q in range(16)], 2)
    return W


@pytest.fixture(scope="module")
def A(oracle):
    W = world_a(oracle)
    yield W
    W.ix.close()


def kinds_batch():
    """16 queries: each kind alone; phrase and term groups together with min_should 0, 1, 2 and groups + 1; two
    variants where only the second can match; a variant absent from one segment; every variant absent under MUST
    and under MUST_NOT; a group with zero variants; queries without a group"""
    return [
        ([], [must([0, 1])], 0),
        ([], [must([0, 1], kind=SHOULD)], 1),
        ([], [must([0, 1], kind=MUST_NOT)], 0),
        ([(SHOULD, [2]), (MUST_NOT, [5, 7])], [must([0, 1], slop=2), must([1, 0], kind=SHOULD)], 1),
        ([(SHOULD, [1]), (SHOULD, [2])], [must([0, 0], kind=SHOULD), must([1, 2], kind=SHOULD, slop=3)], 0),
        ([(SHOULD, [1]), (SHOULD, [2])], [must([0, 0], kind=SHOULD), must([1, 2], kind=SHOULD, slop=3)], 1),
        ([(SHOULD, [1]), (SHOULD, [2])], [must([0, 0], kind=SHOULD), must([1, 2], kind=SHOULD, slop=3)], 2),
        ([(SHOULD, [1]), (SHOULD, [2])], [must([0, 0], kind=SHOULD), must([1, 2], kind=SHOULD, slop=3)], 5),  # groups + 1
        ([], [must([11, 10, 9, 8], [0, 1])], 0),                      # only the second variant matches
        ([], [must([(0, NO_TERM), (1, 1)])], 0),                      # absent from segment 1: no row of it
        ([], [must([(0, NO_TERM), 1], [(NO_TERM, 0), 2])], 0),        # one variant per segment
        ([], [must([(NO_TERM, NO_TERM), 1])], 0),                     # every variant absent: MUST rejects all
        ([], [must([(NO_TERM, NO_TERM), 1], kind=MUST_NOT)], 0),      # ... MUST_NOT rejects nothing
        ([], [(MUST, 0, [])], 0),                                     # a group with zero variants
        ([], [], 0),                                                  # no group
        ([(MUST, [1])], [must([0, 0, 0], slop=4, kind=MUST_NOT), must([1], kind=SHOULD)], 1),
    ]


@pytest.mark.parametrize("k", KS)
def test_kinds_variants_and_mixing(A, k):
    got = A.check(A.qs, kinds_batch(), k, f"kinds k={k}")
    cnt = got[3]
    assert cnt[0] > 0 and cnt[1] == cnt[0] and cnt[2] > 0 and cnt[7] == 0 and cnt[8] == cnt[0]
    assert cnt[4] >= cnt[5] >= cnt[6] and cnt[11] == 0 and cnt[13] == 0 and cnt[12] > 0 and cnt[14] > 0
    assert cnt[9] > 0 and not (got[1][9, :cnt[9]] == 1).any()
    if k == 1025:
        assert {0, 1} <= set(got[1][10, :cnt[10]].tolist()) and cnt[4] > cnt[5] > cnt[6] > 0


def test_32_groups(A):
    """12 term groups and 20 phrase groups: the last phrase group is bit 31"""
    tg = [(SHOULD, [t]) for t in range(12)]
    ph = [must([a, b], kind=SHOULD, slop=1) for a in range(4) for b in range(5)]
    assert len(tg) + len(ph) == 32
    ph[-1] = must([0, 1])  # MUST on bit 31
    queries = [(tg, ph, ms) for ms in (0, 3, 8, 31)] + [([], [], 0)] * 12
    got = A.check(A.qs, queries, 1025, "32 groups")
    assert got[3][0] >= got[3][1] > got[3][2] > 0 and got[3][3] == 0


def test_a_segment_without_positions(oracle):
    """positions set for segment 0 only: no phrase holds a doc of segment 1 — MUST keeps none of it, MUST_NOT all"""
    W = world_a(oracle, positions_for=(0,))
    try:
        got = W.check(W.qs, kinds_batch(), 1025, "no positions in segment 1")
        assert got[3][0] > 0 and not (got[1][0, :got[3][0]] == 1).any()
        assert (got[1][2, :got[3][2]] == 1).any()
    finally:
        W.ix.close()


def test_filter_on_top(A):
    rng = np.random.default_rng(31)
    masks = [rng.random(s.n_docs) < 0.5 for s in A.segs]
    fid = A.ix.add_filter(masks)
    try:
        qf = np.where(np.arange(16) % 2 == 0, fid, -1).astype(np.int32)
        got = A.check(A.qs, kinds_batch(), 1025, "filter on top", q_filter=qf, filters={fid: masks})
        plain = A.check(A.qs, kinds_batch(), 1025, "no filter")
        assert got[3][0] < plain[3][0] and got[3][14] < plain[3][14] and np.array_equal(got[3][1::2], plain[3][1::2])
    finally:
        A.ix.remove_filter(fid)


def test_field_sort_with_matched_counts(A):
    rng = np.random.default_rng(41)
    vals = [[[int(rng.integers(0, 8))] for _ in range(s.n_docs)] for s in A.segs]
    fields = {"low": (vals, False)}
    fid = A.ix.add_sort_field(vals, np.int64)
    try:
        cl, ph = specs_of(kinds_batch(), 2)
        k_all = sum(s.n_docs for s in A.segs)
        want_all = P.reference(A.oracle, A.segs, *A.qs, k_all, ph, clauses=cl)
        for order in ("asc", "desc"):
            sort = [("low", order), ("_score", "desc")]
            for k in (11, 257):
                got = A.ix.search_batch_phrase(*A.qs, k, ph, clauses=cl, sort=[(fid, order), ("_score", "desc")])
                check_sorted(got, expected_rows(want_all, sort, fields), k, sort, f"sorted {order} k={k}")
        assert got[4][7] == 0 and got[4][11] == 0 and got[4][0] > 0
    finally:
        A.ix.remove_sort_field(fid)


def test_plans_and_the_many_term_kernel(A):
    """a flat DisMax plan, and 12 scored lists on the many-term kernel"""
    nq = 16
    flat = dict(q_leaf=np.tile([0, 0, 1], nq), q_plan=np.full(nq, 1, np.int32), q_tie=np.full(nq, 0.3, F32))
    A.check(A.qs, kinds_batch(), 257, "flat DisMax", **flat)
    qs = csr([[(t, 1.0 + 0.1 * t) for t in range(12)] for _ in range(4)], 2)
    many = [([(SHOULD, [t]) for t in range(1, 6)], [must([0, 1], slop=q)], 2 + q) for q in range(4)]
    for k in (11, 1025):
        got = A.check(qs, many, k, f"12 lists k={k}")
    assert got[3][0] > got[3][3] > 0


def test_run_twice_and_batches_in_flight(A, T):
    """slg_batch_run twice on one batch gives the same rows; two batches in flight on their own streams"""
    import torch
    k = 257
    cl, ph = specs_of(kinds_batch(), 2)
    want = P.reference(A.oracle, A.segs, *A.qs, k, ph, clauses=cl)
    sd = P.scored_docs(A.segs, A.qs[0], A.qs[1], ph, cl).tolist()
    b = A.ix.prepare(*A.qs, k, clauses=cl, phrases=ph)
    for _ in range(2):
        b.run()
        got = b.fetch(want_stats=True)
        same(got, want, "run again")
        assert [int(got[4][q].scored_docs) for q in range(16)] == sd
    b.close()
    qs = csr([[(ALL, 1.0), (int(t), 0.5)] for t in (3, 5)], 1)
    specs = [specs_of([([], [must([ALL, 2], slop=2)], 0), ([], [must([1, 2], kind=MUST_NOT)], 0)], 1),
             specs_of([([], [must([2, 1], kind=MUST_NOT)], 0), ([], [must([3], kind=SHOULD), must([X, Y], kind=SHOULD)], 1)], 1)]
    wants = [P.reference(T.oracle, T.segs, *qs, k, p, clauses=c) for c, p in specs]
    streams = [torch.cuda.Stream() for _ in specs]
    batches = [T.ix.prepare(*qs, k, clauses=c, phrases=p) for c, p in specs]
    for bb, s in zip(batches, streams):
        bb.set_stream(s.cuda_stream)
    for _ in range(3):
        for bb in batches:
            bb.run()
    for bb, w in zip(batches, wants):
        same(bb.fetch(), w, "in flight")
        bb.close()


def test_batch_keeps_its_index_state(oracle):
    """a phrase batch prepared before slg_index_update_deleted, and one prepared before slg_index_set_positions
    replaces the segment's positions, answer against the state they were prepared on; update_deleted keeps the
    positions, NULL / NULL removes them"""
    W = world_a(oracle, seed=13, tuning={"updatable": 1})
    try:
        rng, k = W.rng, 33
        cl, ph = specs_of(kinds_batch(), 2)
        old = [copy.copy(s) for s in W.segs]
        want_old = P.reference(oracle, old, *W.qs, k, ph, clauses=cl)
        b = W.ix.prepare(*W.qs, k, clauses=cl, phrases=ph)
        bm = dead_bitmap(rng, 300, 0.3)
        W.ix.update_deleted(0, bm, 300.0 - float(np.unpackbits(bm, bitorder="little")[:300].sum()))
        b.run()
        same(b.fetch(), want_old, "prepared before the update")
        b.close()
        want_new = P.reference(oracle, W.ix.segments, *W.qs, k, ph, clauses=cl)
        same(W.ix.search_batch_phrase(*W.qs, k, ph, clauses=cl), want_new, "after the update: positions kept")
        assert not np.array_equal(want_new[0], want_old[0])
        # new positions for segment 1: every position doubled (adjacent tokens are now a gap of one apart)
        b = W.ix.prepare(*W.qs, k, clauses=cl, phrases=ph)
        seg1 = W.ix.segments[1]
        W.ix.set_positions(1, seg1.pos_offsets, seg1.positions * 2)
        b.run()
        same(b.fetch(), want_new, "prepared before the positions were replaced")
        b.close()
        want_doubled = P.reference(oracle, W.ix.segments, *W.qs, k, ph, clauses=cl)
        same(W.ix.search_batch_phrase(*W.qs, k, ph, clauses=cl), want_doubled, "after the positions were replaced")
        assert not np.array_equal(want_doubled[0][0], want_new[0][0])
        W.ix.set_positions(1, None, None)
        want_none = P.reference(oracle, W.ix.segments, *W.qs, k, ph, clauses=cl)
        got = W.ix.search_batch_phrase(*W.qs, k, ph, clauses=cl)
        same(got, want_none, "after the positions were removed")
        assert not (got[1][0, :got[3][0]] == 1).any()
    finally:
        W.ix.close()


def test_one_call_form_and_refusals(A):
    """slg_search_batch_phrase = prepare + run + fetch; a phrase batch does not run sharded; q_min_match > 1, a
    q_min_should in the bool spec and a term id beyond a segment's vocabulary are invalid; bad positions are
    refused; the other batch kinds take no phrases"""
    import ctypes as C
    from searchlite_amd import _native as N, searcher
    W, k = A, 11
    cl, ph = specs_of(kinds_batch(), 2)
    pspec, keep_p = searcher.phrase_spec(ph, 16)
    bspec, keep_b = searcher.bool_spec(cl, 16)
    o, t, w = (np.ascontiguousarray(a) for a in W.qs)
    outs = [np.zeros((16, k), dt) for dt in (np.uint32, np.uint32, F32)] + [np.zeros(16, np.uint32)]
    stats = (N.Stats * 16)()
    N.check(W.ix._lib.slg_search_batch_phrase(W.ix._h, 16, o.ctypes.data, t.ctypes.data, w.ctypes.data, None, None, None,
                                              C.addressof(bspec), C.addressof(pspec), k, 1,
                                              *[a.ctypes.data for a in outs], C.addressof(stats), None))
    same(tuple(outs), P.reference(W.oracle, W.segs, *W.qs, k, ph, clauses=cl), "one call")
    assert [int(s.scored_docs) for s in stats] == P.scored_docs(W.segs, o, t, ph, cl).tolist()
    b = W.ix.prepare(*W.qs, k, clauses=cl, phrases=ph)
    try:
        group = searcher.ShardGroup(W.ix, 0, 1, searcher.shard_unique_id(), 2)
        try:
            with pytest.raises(N.SlgError) as ei:
                b.run_sharded(group)
            assert ei.value.code == N.ERR_UNSUPPORTED and "phrase" in ei.value.msg
            with pytest.raises(N.SlgError) as ei:
                b.fetch_sharded()
            assert ei.value.code == N.ERR_UNSUPPORTED
        finally:
            group.close()
    finally:
        b.close()
    with pytest.raises(N.SlgError) as ei:
        W.ix.prepare(*W.qs, k, phrases=ph, q_min_match=np.full(16, 2, np.uint32))
    assert ei.value.code == N.ERR_INVALID and "q_min_match" in ei.value.msg
    with pytest.raises(N.SlgError) as ei:
        W.ix.prepare(*W.qs, k, phrases=ph, clauses=dict(cl, q_min_should=1))
    assert ei.value.code == N.ERR_INVALID and "q_min_should" in ei.value.msg
    with pytest.raises(N.SlgError) as ei:
        W.ix.prepare(*W.qs, k, phrases=dict(ph, t_terms=np.full_like(ph["t_terms"], 12345)))
    assert ei.value.code == N.ERR_INVALID and "term id out of range" in ei.value.msg
    seg = W.segs[1]
    bad = seg.positions.copy()
    a = int(np.argmax(np.diff(seg.pos_offsets.astype(np.int64)) >= 2))  # a posting with two positions
    bad[int(seg.pos_offsets[a])] = bad[int(seg.pos_offsets[a]) + 1] + 1
    for po, ps, word in ((seg.pos_offsets, bad, "decrease"), (seg.pos_offsets[::-1], seg.positions, "pos_offsets"),
                         (seg.pos_offsets, seg.positions | np.uint32(1 << 31), "2^31")):
        with pytest.raises(N.SlgError) as ei:
            W.ix.set_positions(1, po, ps)
        assert ei.value.code == N.ERR_INVALID and word in ei.value.msg
    with pytest.raises(N.SlgError):
        W.ix.set_positions(2, seg.pos_offsets, seg.positions)
    W.check(W.qs, kinds_batch(), k, "after the refused updates")  # the index is as it was
    for other in (dict(hybrid=True), dict(cursors=[None] * 16)):
        with pytest.raises(N.SlgError) as ei:
            W.ix.prepare(*W.qs, k, phrases=ph, **other)
        assert ei.value.code == N.ERR_UNSUPPORTED


@pytest.mark.parametrize("k", (11, 1025))
def test_bool_and_plain_batches_are_unchanged(oracle, A, k):
    """regression guard on the same index: a bool batch still equals bool_ref, a plain batch the oracle, and a phrase
    batch whose queries have no group equals the plain batch"""
    tg = [(tgs, 1) for tgs, _, _ in kinds_batch()]
    cl = B.clauses_of(tg, 2)
    same(A.ix.search_batch_bool(*A.qs, k, cl), B.reference(oracle, A.segs, *A.qs, k, cl), f"bool k={k}")
    want = oracle.search_batch(A.segs, *A.qs, k, strategy=oracle.BM25)
    same(A.ix.search_plan(*A.qs, k), want, f"plain k={k}")
    same(A.ix.search_batch_phrase(*A.qs, k, P.phrases_of([([], 0)] * 16, 2)), want, f"no groups k={k}")
