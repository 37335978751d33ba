"""rescore_kernel at the boundaries its own constants create: every register top-k width at its window edges
(lds_rows = (max(window, 2) + 1) & ~1 through kregs_for) and the rows-per-lane steps at 256 r, the largest LDS
layout (1024 rows + 2048 table entries), 64 segments, the f32 rules of negative, overflowing and zero weights,
and the order of additions when the terms of a leaf are interleaved or repeated.

Conventions of tests/test_gpu_rescore.py: tolerance 0, same() over all seven arrays against tests/rescore_ref.py,
rows past the count are zero.  r comes from the oracle's exhaustive run (R.rescore_maps) where the weights are
positive, and from R.direct_maps (the impacts combined as the header states) where they are not; the leaf-order
test takes both and asserts that they agree."""
import numpy as np
import pytest

from tests import rescore_ref as R
from tests.test_gpu_rescore import F32, NO_TERM, csr, dead_bitmap, same
from tests.util import _append_lists, random_queries, random_segment

pytestmark = pytest.mark.gpu
K_WIDE = 1025
# lds_rows / kregs of each window: 2 -> 2 / 1; 63 -> 64 / 1; 127 -> 128 / 2; 128 -> 128 / 2; 129 -> 130 / 4;
# 130 -> 130 / 4; 255 -> 256 / 4; 511 -> 512 / 8; 512 -> 512 / 8; 513 -> 514 / 16; 767, 768, 769 -> 16 (the third
# row of a lane ends at 768); 1023 -> 1024 / 16
WINDOWS = (2, 63, 127, 128, 129, 130, 255, 511, 512, 513, 767, 768, 769, 1023)
MIXED_WINDOWS = (1, 129, 513, 1024, 129)


def spec(queries, n_segs, **kw):
    return dict(zip(("q_offsets", "q_terms", "q_weights"), csr(queries, n_segs)), **kw)


class Edge:
    """an index, its segments and the first passes computed so far"""

    def __init__(self, sa, oracle, segs):
        self.oracle, self.segs, self.ix = oracle, segs, sa.GpuIndex(segs)
        self._first, self._maps = {}, {}

    def first(self, name, qs, k, **plans):
        if (name, k) not in self._first:
            self._first[name, k] = R.first_pass(self.oracle, self.segs, *qs, k, **plans)
        return self._first[name, k]

    def maps(self, name, rescore, direct):
        if name not in self._maps:
            self._maps[name] = (R.direct_maps if direct else R.rescore_maps)(self.oracle, self.segs, rescore)
        return self._maps[name]

    def check(self, qname, qs, k, rname, rescore, what, direct=False, ref_plans=None, **plans):
        """one rescore batch against the reference -> (got, the window of every query)"""
        got = self.ix.search_rescore(*qs, k, rescore, **plans)
        first = self.first(qname, qs, k, **dict(plans, **(ref_plans or {})))
        want = R.rescore_batch(first, self.maps(rname, rescore, direct), rescore["window"], rescore.get("mode"))
        same(got, want, what)
        nq = len(got[3])
        return got, np.minimum(R.per_query(rescore["window"], nq, 0), got[3])


def some_rescored_some_not(got, w, what):
    flag = got[6]
    inside = np.arange(flag.shape[1])[None, :] < np.asarray(w)[:, None]
    assert (flag[inside] == 1).any(), f"{what}: no row was rescored"
    assert (flag[inside] == 0).any(), f"{what}: every window row was rescored"
    assert not flag[~inside].any()


# ---- 1. widths and rows per lane --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(oracle):
    """one segment of 3000 docs; appended lists: one in every doc (count == k), df 1, 64, 65 and 2000 whose first
    and last postings are docs 0 and 2999, and a list that puts docs 0, 7, 1500, 2500 and 2999 on top of the first
    pass, so the ends are rows of every window"""
    import searchlite_amd as sa
    rng = np.random.default_rng(101)
    n, vocab = 3000, 40
    base = random_segment(rng, n, vocab, 6)
    ends = np.array([0, n - 1], np.uint32)

    def with_ends(df):
        inner = rng.choice(np.arange(1, n - 1), size=df - 2, replace=False)
        return np.sort(np.concatenate([ends, inner.astype(np.uint32)]))

    lists = {"all": np.arange(n, dtype=np.uint32), "top": np.array([0, 7, 1500, 2500, n - 1], np.uint32),
             "one": np.array([1234], np.uint32), "d64": with_ends(64), "d65": with_ends(65), "d2000": with_ends(2000)}
    seg = _append_lists(base, [(d, rng.integers(1, 4, size=len(d))) for d in lists.values()])
    T = {name: vocab + i for i, name in enumerate(lists)}
    W = Edge(sa, oracle, [seg])
    W.qs = csr([[(T["all"], 1.0), (T["top"], 5.0), (int(rng.integers(0, vocab)), 0.5)] for _ in range(5)], 1)
    # query 0 rescores every row, query 1 at most one (doc 1234): every case has rescored rows and others
    W.rescore = spec([[(T["all"], 0.5)], [(T["one"], 3.0)], [(T["d64"], 1.0), (T["d65"], 2.0)],
                      [(T["d2000"], 1.0), (T["all"], 0.25), (T["d64"], 4.0)], [(T["d2000"], 2.0), (T["one"], 1.0)]], 1)
    yield W
    W.ix.close()


def check_wide(W, window, mode, what):
    got, w = W.check("wide", W.qs, K_WIDE, "wide", dict(W.rescore, window=window, mode=mode), what)
    assert np.all(got[3] == K_WIDE), "the every-doc list fills the k rows"
    assert np.array_equal(w, np.minimum(R.per_query(window, len(w), 0), K_WIDE))
    some_rescored_some_not(got, w, what)
    return got, w


@pytest.mark.parametrize("window", WINDOWS)
def test_window_matrix(wide, window):
    """one batch per window: the window picks lds_rows, the register width and how many of a lane's four rows
    are live"""
    got, w = check_wide(wide, window, R.TOTAL, f"window {window}")
    doc, flag = got[0], got[6]
    if window >= 63:  # docs 0 and 2999 lead the first pass: rows of the window, first and last posting of d64 / d65
        for q in (2, 3):
            for d in (0, 2999):
                i = np.nonzero(doc[q, :window] == d)[0]
                assert len(i) == 1 and flag[q, i[0]] == 1, (window, q, d)


def test_mixed_windows_in_one_batch(wide):
    """windows 1, 129, 513, 1024 in one batch: 1024 picks the kernel, the others run wider than they need; every
    score mode"""
    check_wide(wide, np.array(MIXED_WINDOWS), np.arange(5) % 5, "mixed windows")
    check_wide(wide, np.array(MIXED_WINDOWS[::-1]), R.MULTIPLY, "mixed windows, reversed")


# ---- 2. the largest table, 64 segments ----------------------------------------------------------------------
N_SEGS, N_TERMS = 64, 32


def many_segments(rng, n_segs, vocab=34):
    """segments of 30-49 docs, vocabulary 34 + a list in every doc (term 34); tombstones in two of them"""
    segs = []
    for s in range(n_segs):
        n = int(rng.integers(30, 50))
        base = random_segment(rng, n, vocab, 6, zipf=False)
        segs.append(_append_lists(base, [(np.arange(n, dtype=np.uint32), rng.integers(1, 4, size=n))]))
    for s in (3, n_segs - 1):
        segs[s].deleted = dead_bitmap(rng, segs[s].n_docs, 0.2)
    return segs


def table_queries(rng, n_segs, n_terms, vocab=34, nq=4):
    """first pass: the every-doc term and one more; rescore: n_terms distinct terms per query, a tenth of the
    table NO_TERM, query 1 on 8 leaves under DisMax 0.3, query 2 with min_match 3"""
    fq = csr([[(vocab, 1.0), (int(rng.integers(0, vocab)), 0.5 + 0.25 * q)] for q in range(nq)], n_segs)
    rq = [[(int(t), float(F32(0.25 + 0.125 * i))) for i, t in enumerate(rng.permutation(vocab)[:n_terms])]
          for _ in range(nq)]
    rs = spec(rq, n_segs)
    rs["q_terms"][rng.random(rs["q_terms"].shape) < 0.1] = NO_TERM
    leaf = np.tile(np.arange(n_terms), nq)
    leaf[n_terms:2 * n_terms] = np.arange(n_terms) % 8
    rs.update(q_leaf=leaf.astype(np.uint32), q_plan=np.array([0, 1, 0, 0], np.int32), q_tie=np.full(nq, 0.3, F32),
              q_min_match=np.array([0, 0, 3, 0], np.uint32), window=1024, mode=np.arange(nq) % 5)
    return fq, rs


@pytest.fixture(scope="module")
def many(oracle):
    import searchlite_amd as sa
    rng = np.random.default_rng(202)
    W = Edge(sa, oracle, many_segments(rng, N_SEGS))
    W.qs, W.rescore = table_queries(rng, N_SEGS, N_TERMS)
    yield W
    W.ix.close()


def test_largest_table_and_window(many):
    """32 terms x 64 segments = 2048 table entries behind 1024 rows: the 61 440-byte layout; rows of every
    segment are looked up in their own column of the table"""
    from searchlite_amd import _native as N
    assert N_TERMS == N.MAX_QUERY_TERMS and N_TERMS * N_SEGS == 2048
    assert int(np.diff(many.rescore["q_offsets"]).max()) * many.rescore["q_terms"].shape[1] == 2048
    assert (many.rescore["q_terms"] == NO_TERM).any()
    got, w = many.check("many", many.qs, K_WIDE, "many", many.rescore, "2048 entries, window 1024")
    assert np.all(got[3] == K_WIDE) and np.all(w == 1024)
    flag, seg = got[6], got[1]
    assert flag[:, :1024].any() and not flag[:, 1024:].any()
    assert (flag[2, :1024] == 0).any(), "min_match 3 leaves some rows as they are"
    assert len(set(seg[flag == 1].tolist())) == N_SEGS, "rescored rows of every segment"


def test_refusals_above_the_table_and_term_limits(oracle, many):
    from searchlite_amd import _native as N
    import searchlite_amd as sa
    rng = np.random.default_rng(203)
    # 33 rescore terms in a query: invalid
    fq, rs33 = table_queries(rng, N_SEGS, 33)
    with pytest.raises(N.SlgError) as ei:
        many.ix.search_rescore(*many.qs, K_WIDE, rs33)
    assert ei.value.code == N.ERR_INVALID
    # 65 segments x 32 terms = 2080 entries: unsupported, refused before any launch
    W = Edge(sa, oracle, many_segments(rng, N_SEGS + 1))
    try:
        qs, rs = table_queries(rng, N_SEGS + 1, N_TERMS)
        with pytest.raises(N.SlgError) as ei:
            W.ix.search_rescore(*qs, K_WIDE, rs)
        assert ei.value.code == N.ERR_UNSUPPORTED and "table entries" in ei.value.msg
        # 31 terms x 65 segments = 2015: a valid batch on the same index afterwards
        qs, rs = table_queries(rng, N_SEGS + 1, 31)
        got, w = W.check("65", qs, K_WIDE, "65", rs, "31 terms x 65 segments")
        assert got[6].any() and np.all(w == 1024)
    finally:
        W.ix.close()
    got, w = many.check("many", many.qs, K_WIDE, "many", many.rescore, "after the refusals")
    assert got[6].any()


# ---- 3. f32 edges ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(oracle):
    """two segments of 300 and 200 docs, vocabulary 40, tombstones in one; 16 first-pass queries of three terms
    with positive weights (qs) and with weights of both signs (qs_signed)"""
    import searchlite_amd as sa
    rng = np.random.default_rng(303)
    segs = [random_segment(rng, 300, 40, 6), random_segment(rng, 200, 40, 6)]
    segs[1].deleted = dead_bitmap(rng, 200, 0.15)
    W = Edge(sa, oracle, segs)
    W.qs = random_queries(rng, 16, 3, 40, n_segs=2, weights=True)
    o, t, w = W.qs
    W.qs_signed = (o, t, (w * np.where(np.arange(len(w)) % 3 == 1, -1.0, 1.0)).astype(F32))
    W.pick = lambda n: [int(x) for x in rng.choice(12, size=n, replace=False)]  # (common terms: many rows match)
    yield W
    W.ix.close()


def two_leaf_queries(W, w0, w1, **kw):
    """16 rescore queries of two terms on two leaves with weights w0, w1"""
    return spec([[(t, w) for t, w in zip(W.pick(2), (w0, w1))] for _ in range(16)], 2, **kw)


F32_CASES = {
    # negative rescore weights under Sum: the sum starts at -0.0 and goes below 0
    "negative_sum_total": (lambda W: two_leaf_queries(W, -1.5, -0.75), R.TOTAL, "qs"),
    "negative_sum_multiply": (lambda W: two_leaf_queries(W, -1.5, 0.5), R.MULTIPLY, "qs"),
    # DisMax 0.3 of negative leaves: with both leaves named and held, the max is the less negative leaf; where a
    # leaf is missing (a doc that one list holds, a leaf absent from segment 1, a third leaf nothing names) 0.0
    # joins the max
    "negative_dismax": (lambda W: two_leaf_queries(W, -1.5, -0.75, q_plan=1, q_tie=F32(0.3)), R.TOTAL, "qs"),
    "negative_dismax_missing_leaf": (lambda W: two_leaf_queries(W, -1.5, -0.75, q_plan=1, q_tie=F32(0.3), q_nleaves=3),
                                     R.TOTAL, "qs"),
    "negative_dismax_leaf_absent_from_a_segment": (lambda W: absent_in_segment_1(
        two_leaf_queries(W, -1.5, -0.75, q_plan=1, q_tie=F32(0.3))), R.MIN, "qs"),
    # +-3e38: impact * weight overflows where the impact is above 1.13, r is +-inf, or NaN where both leaves hold
    # the doc; total adds it, max / min meet a NaN operand, multiply meets first-pass scores of both signs
    "overflow_total": (lambda W: two_leaf_queries(W, 3e38, -3e38), R.TOTAL, "qs"),
    "overflow_max": (lambda W: two_leaf_queries(W, 3e38, -3e38), R.MAX, "qs"),
    "overflow_min": (lambda W: two_leaf_queries(W, 3e38, -3e38), R.MIN, "qs"),
    "overflow_multiply_signed_first_pass": (lambda W: two_leaf_queries(W, 3e38, -3e38), R.MULTIPLY, "qs_signed"),
    "negative_multiply_signed_first_pass": (lambda W: two_leaf_queries(W, -1.5, 0.5), R.MULTIPLY, "qs_signed"),
    # weight 0: r = +0.0; under total every matched row keeps its exact score (and its exact ties), under
    # multiply the rows become +0.0 and -0.0 by the sign of their first-pass score
    "zero_total": (lambda W: two_leaf_queries(W, 0.0, 0.0), R.TOTAL, "qs"),
    "zero_multiply_signed_first_pass": (lambda W: two_leaf_queries(W, 0.0, 0.0), R.MULTIPLY, "qs_signed"),
}


def absent_in_segment_1(rs):
    rs["q_terms"] = rs["q_terms"].copy()
    rs["q_terms"][1::2, 1] = NO_TERM  # leaf 1 has no term in segment 1
    return rs


@pytest.mark.parametrize("name", list(F32_CASES))
def test_f32_edges(oracle, small, name):
    W = small
    make, mode, qname = F32_CASES[name]
    rescore = dict(make(W), window=64, mode=mode)
    # (the first pass of the signed queries: the oracle's brute-force scorer)
    ref_plans = dict(strategy=oracle.BM25) if qname == "qs_signed" else None
    got, w = W.check(qname, getattr(W, qname), 65, name, rescore, name, direct=True, ref_plans=ref_plans)
    doc, seg, score, count, first, rsc, flag = got
    inside = np.arange(65)[None, :] < w[:, None]
    hit = inside & (flag == 1)
    assert hit.any() and (inside & (flag == 0)).any()
    if name.startswith("negative"):
        assert (rsc[hit] < 0).any()
    if name == "negative_dismax_missing_leaf":  # 0.0 is every row's max: r = 0.3 x the negative sum
        assert (rsc[hit] < 0).all()
    if name.startswith("overflow"):
        assert np.isinf(rsc[hit]).any() and np.isnan(rsc[hit]).any() and np.isfinite(rsc[hit]).any()
    if name == "overflow_total":
        assert np.isnan(score[inside]).any() and (score[inside] == np.inf).any() and (score[inside] == -np.inf).any()
    if name in ("overflow_max", "overflow_min"):
        nan_r = hit & np.isnan(rsc)
        assert np.array_equal(score[nan_r].view(np.uint32), first[nan_r].view(np.uint32)), "a NaN r yields the first score"
    if name.endswith("signed_first_pass"):
        assert (first[hit] < 0).any() and (first[hit] > 0).any()
    if name == "zero_total":
        assert np.array_equal(score.view(np.uint32), first.view(np.uint32)) and not rsc.any()
        assert not np.signbit(rsc[hit]).any()
    if name == "zero_multiply_signed_first_pass":
        z = score[hit]
        assert np.all(z == 0) and np.signbit(z).any() and (~np.signbit(z)).any()


# ---- 4. leaf order --------------------------------------------------------------------------------------------
def leaf_order_queries(W):
    a = [W.pick(4) for _ in range(16)]
    ws = (0.7, 1.3, 2.9, 0.11)  # four distinct weights
    return {
        # leaf 0 = terms 1 and 3, leaf 1 = terms 0 and 2, each in query-term order
        "interleaved": spec([[(t, w) for t, w in zip(q, ws)] for q in a], 2, q_leaf=np.tile([1, 0, 1, 0], 16)),
        # term x twice in leaf 0, between them another term: x w0 + y w1 + x w2
        "twice_in_one_leaf": spec([[(q[0], ws[0]), (q[1], ws[1]), (q[0], ws[2]), (q[2], ws[3])] for q in a], 2,
                                  q_leaf=np.tile([0, 0, 0, 1], 16)),
        # term x in leaf 0 and in leaf 1
        "in_two_leaves": spec([[(q[0], ws[0]), (q[1], ws[1]), (q[0], ws[2]), (q[2], ws[3])] for q in a], 2,
                              q_leaf=np.tile([0, 0, 1, 1], 16)),
    }


@pytest.mark.parametrize("plan", ["sum", "dismax"])
@pytest.mark.parametrize("name", ["interleaved", "twice_in_one_leaf", "in_two_leaves"])
def test_leaf_order(oracle, small, name, plan):
    W = small
    if not hasattr(W, "leaf_queries"):
        W.leaf_queries = leaf_order_queries(W)
    rescore = dict(W.leaf_queries[name], window=64, mode=R.TOTAL, q_min_match=2)
    if plan == "dismax":
        rescore.update(q_plan=1, q_tie=F32(0.3))
    tag = f"{name}/{plan}"
    got, w = W.check("qs", W.qs, 65, tag, rescore, tag, direct=True)
    inside = np.arange(65)[None, :] < w[:, None]
    assert (inside & (got[6] == 1)).any() and (inside & (got[6] == 0)).any(), "min_match 2 holds some rows, not all"
    # the oracle's exhaustive run adds in the same order: both references agree on the live docs
    dead = [None if s.deleted is None else np.unpackbits(s.deleted, bitorder="little") for s in W.segs]
    for a, b in zip(R.rescore_maps(oracle, W.segs, rescore), W.maps(tag, rescore, True)):
        live = {k: v for k, v in b.items() if dead[k[0]] is None or not dead[k[0]][k[1]]}
        assert {k: F32(v).tobytes() for k, v in a.items()} == {k: F32(v).tobytes() for k, v in live.items()}, tag
