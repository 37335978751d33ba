"""Boolean queries on the device (slg_batch_prepare_bool, slg_search_batch_bool) through the C ABI against
tests/bool_ref.py.  Tolerance 0: docs, segments, scores (bit patterns), counts, scored_docs and matched counts are
identical to the reference; rows past the count are zero."""
import copy

import numpy as np
import pytest

from tests import bool_ref as B
from tests.test_gpu_sort import check as check_sorted, expected_rows
from tests.util import _append_lists, random_queries, random_segment

pytestmark = pytest.mark.gpu
F32 = np.float32
NO_TERM = 0xFFFFFFFF
MUST, SHOULD, MUST_NOT = B.MUST, B.SHOULD, B.MUST_NOT
KS = (1, 11, 257, 1025)


def same(got, want, what):
    for name, g, w in zip(("doc", "seg", "score", "count"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {name} shape {g.shape} != {w.shape}"
        gb, wb = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == F32 else (g, w)
        if not np.array_equal(gb, wb):
            q, i = (np.argwhere(gb != wb)[0].tolist() + [0])[:2]
            raise AssertionError(f"{what}: {name} differs at query {q} row {i}: {g[q] if g.ndim == 1 else g[q, i]!r} "
                                 f"!= {w[q] if w.ndim == 1 else w[q, i]!r}")
    doc, seg, score, count = got[:4]
    for q in range(len(count)):  # rows past the count are zero
        n = int(count[q])
        assert not (doc[q, n:].any() or seg[q, n:].any() or score[q, n:].any()), f"{what}: query {q} has rows past its count"


def dead_bitmap(rng, n, p):
    return np.packbits(rng.random(n) < p, bitorder="little")


def csr(queries, n_segs):
    """[[(term ids per segment or one id, weight)]] -> (q_offsets, q_terms [total, n_segs], q_weights)"""
    offs, terms, ws = [0], [], []
    for q in queries:
        for t, w in q:
            terms.append([t] * n_segs if np.ndim(t) == 0 else list(t))
            ws.append(w)
        offs.append(len(ws))
    return np.array(offs, np.uint32), np.array(terms, np.uint32).reshape(-1, n_segs), np.array(ws, F32)


class World:
    def __init__(self, sa, oracle, segs, **tuning):
        self.oracle, self.segs = oracle, segs
        self.ix = sa.GpuIndex(segs, **tuning)
        self.n_segs = len(segs)

    def check(self, qs, queries, k, what, **kw):
        """a bool batch of `queries` (bool_ref.clauses_of) over the scored queries qs, with stats -> got"""
        cl = B.clauses_of(queries, self.n_segs)
        flt = {n: kw.pop(n) for n in ("q_filter", "filters") if n in kw}
        got = self.ix.search_batch_bool(*qs, k, cl, want_stats=True, q_filter=flt.get("q_filter"), **kw)
        want = B.reference(self.oracle, self.segs, *qs, k, cl, **flt, **kw)
        same(got, want, what)
        sd = B.scored_docs(self.segs, qs[0], qs[1], cl)
        got_sd = [int(got[4][q].scored_docs) for q in range(len(sd))]
        assert got_sd == sd.tolist(), f"{what}: scored_docs {got_sd} != {sd.tolist()}"
        assert [int(got[4][q].candidates_examined) for q in range(len(sd))] == sd.tolist()
        return got


@pytest.fixture(scope="module")
def A(oracle):
    """two segments of 300 and 200 docs, vocab 40, tombstones in both; 16 three-term queries"""
    import searchlite_amd as sa
    rng = np.random.default_rng(17)
    segs = [random_segment(rng, 300, 40, 6), random_segment(rng, 200, 40, 6)]
    segs[0].deleted = dead_bitmap(rng, 300, 0.1)
    segs[1].deleted = dead_bitmap(rng, 200, 0.15)
    W = World(sa, oracle, segs)
    W.qs = random_queries(rng, 16, 3, 40, n_segs=2, weights=True)
    W.rng = rng
    yield W
    W.ix.close()


def scored_terms(W, q):
    o, t, _ = W.qs
    return [int(x) for x in t[int(o[q]):int(o[q + 1]), 0]]


@pytest.fixture(scope="module")
def Bw(oracle):
    """one segment of 6000 docs with appended lists.  Clause lists of df 1, 64, 65, 4096 and 6000 whose first and
    last postings (docs 0 and 5999; 4321 for the df 1 list) are candidates: the binary-search edges.  Scored lists
    of 1, 63, 64, 65 and 129 docs, and subsets of the 129 that leave 0, 1, 63, 64, 65 of them: the chunk edges of
    the compaction."""
    import searchlite_amd as sa
    rng = np.random.default_rng(23)
    n, vocab = 6000, 40
    base = random_segment(rng, n, vocab, 6)
    ends = np.array([0, 4321, n - 1], np.uint32)

    def with_ends(df, pool=None):
        pool = np.setdiff1d(np.arange(1, n - 1) if pool is None else pool, ends)
        inner = rng.choice(pool, size=df - len(ends), replace=False)
        return np.sort(np.concatenate([ends, inner.astype(np.uint32)])).astype(np.uint32)

    c129 = with_ends(129)
    lists = {"all": np.arange(n, dtype=np.uint32), "one": np.array([4321], np.uint32), "d64": with_ends(64),
             "d65": with_ends(65), "d4096": with_ends(4096), "even": np.arange(0, n, 2, dtype=np.uint32),
             "c1": np.array([4321], np.uint32), "c63": with_ends(63), "c64": with_ends(64), "c65": with_ends(65),
             "c129": c129}
    others = np.setdiff1d(np.arange(n), c129)
    for m in (63, 64, 65):  # m docs of c129 (its first and last among them) and 500 docs outside it
        lists[f"k{m}"] = np.sort(np.concatenate([with_ends(m, pool=c129), rng.choice(others, 500, replace=False)])).astype(np.uint32)
    lists["none"] = np.sort(rng.choice(others, 700, replace=False)).astype(np.uint32)
    seg = _append_lists(base, [(d, rng.integers(1, 4, size=len(d))) for d in lists.values()])
    W = World(sa, oracle, [seg])
    W.T = {name: vocab + i for i, name in enumerate(lists)}
    W.lists, W.rng = lists, rng
    yield W
    W.ix.close()


def one_term_queries(W, names):
    return csr([[(W.T[nm], 1.0 + 0.25 * i)] for i, nm in enumerate(names)], 1)


def test_chunk_edges_of_the_compaction(Bw):
    """regions of 1, 63, 64, 65, 129 candidates (one slice each) left with 0, 1, 63, 64, 65, 129 survivors"""
    W, T = Bw, Bw.T
    scored = ["c1", "c63", "c64", "c65", "c129", "c129", "c129", "c129", "c129", "c129", "c129"]
    qs = one_term_queries(W, scored)
    queries = [([(MUST, [T["all"]])], 0), ([(MUST, [T["all"]])], 0), ([(SHOULD, [T["none"]]), (SHOULD, [T["all"]])], 1),
               ([(SHOULD, [T["all"]])], 1), ([(MUST, [T["all"]])], 0), ([(MUST_NOT, [T["all"]])], 0),
               ([(MUST, [T["one"]])], 0), ([(MUST, [T["k63"]])], 0), ([(SHOULD, [T["k64"]])], 1),
               ([(MUST, [T["k65"]])], 0), ([(MUST, [T["none"]])], 0)]
    # on the CPU first: the regions and the survivors are what the case is about
    cl = B.clauses_of(queries, 1)
    region = [len(W.lists[nm]) for nm in scored]
    left = B.scored_docs(W.segs, qs[0], qs[1], cl).tolist()
    assert region == [1, 63, 64, 65, 129, 129, 129, 129, 129, 129, 129]
    assert left == [1, 63, 64, 65, 129, 0, 1, 63, 64, 65, 0]
    b = W.ix.prepare(*qs, 11, clauses=cl)
    assert b.info()["n_slices"] == len(scored)  # one slice per query: a region is a slice
    b.close()
    for k in (11, 257):
        got = W.check(qs, queries, k, f"chunk edges k={k}")
        assert got[3].tolist() == [min(x, k) for x in left]


def test_binary_search_edges(Bw):
    """docs 0 and 5999 are the first and last posting of the df 64, 65, 4096 and 6000 lists, doc 4321 the df 1
    list: they are found under MUST (kept) and under MUST_NOT (dropped)"""
    W, T = Bw, Bw.T
    names = ["one", "d64", "d65", "d4096", "all"]
    qs = one_term_queries(W, ["c129"] * (2 * len(names)))
    queries = [([(MUST, [T[nm]])], 0) for nm in names] + [([(MUST_NOT, [T[nm]])], 0) for nm in names]
    got = W.check(qs, queries, 257, "search edges")
    for i, nm in enumerate(names):
        kept, dropped = set(got[0][i, :got[3][i]].tolist()), set(got[0][len(names) + i, :got[3][len(names) + i]].tolist())
        for d in ((4321,) if nm == "one" else (0, 4321, 5999)):
            assert d in kept and d not in dropped, (nm, d)
        assert kept | dropped == set(W.lists["c129"].tolist()) and not (kept & dropped)


def test_many_slices_and_alternating_accepts(Bw):
    """6000 candidates over several slices: all rejected, none rejected, every other one accepted"""
    W, T = Bw, Bw.T
    qs = csr([[(T["all"], 1.0), (int(t), 0.5)] for t in (3, 5, 7, 9)], 1)
    queries = [([(MUST_NOT, [T["all"]])], 0), ([(MUST, [T["all"]])], 0), ([(MUST, [T["even"]])], 0),
               ([(MUST_NOT, [T["even"]]), (SHOULD, [T["d4096"]]), (SHOULD, [T["d64"], T["d65"]])], 1)]
    b = W.ix.prepare(*qs, 11, clauses=B.clauses_of(queries, 1))
    assert b.info()["n_slices"] > 4
    b.close()
    for k in KS:
        got = W.check(qs, queries, k, f"many slices k={k}")
        assert got[3].tolist()[:3] == [0, k, k] and np.all(got[0][2, :k] % 2 == 0)


def kinds_batch(W):
    """16 queries over world A: every kind alone, all three together, a two-term group, min_should 0 / 1 / 2 /
    groups + 1, a MUST group absent from one segment, a MUST_NOT term absent everywhere, no clause table"""
    rng = np.random.default_rng(5)
    pick = lambda n: [int(x) for x in rng.choice(40, size=n, replace=False)]
    st = lambda q: scored_terms(W, q)
    queries = [
        ([(MUST, [st(0)[0]])], 0),
        ([(SHOULD, [st(1)[1]])], 1),
        ([(MUST_NOT, [pick(1)[0]])], 0),
        ([(MUST, [st(3)[0]]), (SHOULD, [st(3)[1]]), (SHOULD, [st(3)[2]]), (MUST_NOT, pick(2))], 1),
        ([(MUST, pick(2))], 0),                                  # a group of two terms
        ([(SHOULD, [t]) for t in st(5)], 0),
        ([(SHOULD, [t]) for t in st(6)], 1),
        ([(SHOULD, [t]) for t in st(7)], 2),
        ([(SHOULD, [t]) for t in st(8)], 4),                     # groups + 1: nothing
        ([(MUST, [(st(9)[0], NO_TERM)])], 0),                    # absent from segment 1: no row of it
        ([(MUST, [(NO_TERM, st(10)[0]), (st(10)[1], NO_TERM)])], 0),
        ([(MUST_NOT, [(NO_TERM, NO_TERM)])], 0),                 # absent everywhere: rejects nothing
        ([], 0),                                                 # no clause table
        ([], 3),
        ([(MUST, [st(14)[0]]), (MUST, [st(14)[1]]), (MUST_NOT, [st(14)[2]])], 0),
        ([(MUST_NOT, [st(15)[0]]), (MUST_NOT, [st(15)[1]]), (MUST_NOT, [st(15)[2]])], 0),  # every candidate rejected
    ]
    return queries


@pytest.mark.parametrize("k", KS)
def test_kinds_in_score_order(A, k):
    got = A.check(A.qs, kinds_batch(A), k, f"kinds k={k}")
    cnt = got[3]
    assert cnt[8] == 0 and cnt[15] == 0 and cnt[12] > 0 and cnt[11] > 0
    assert not (got[1][9, :cnt[9]] == 1).any() and cnt[9] > 0  # the MUST group is absent from segment 1
    if k == 1025:
        assert {0, 1} <= set(got[1][10, :cnt[10]].tolist())


def test_32_groups_and_64_terms(A):
    rng = np.random.default_rng(9)
    two = lambda: [int(x) for x in rng.choice(40, size=2, replace=False)]
    q32 = [(MUST, [scored_terms(A, 0)[0], 39])] + [(MUST_NOT, [(NO_TERM, 38), (37, NO_TERM)])] + \
          [(SHOULD, two()) for _ in range(30)]
    assert len(q32) == 32 and sum(len(t) for _, t in q32) == 64
    queries = [(q32, ms) for ms in (0, 3, 8, 31)] + [([], 0)] * 12
    got = A.check(A.qs, queries, 1025, "32 groups, 64 terms")
    assert got[3][0] > got[3][1] > got[3][2] > 0 and got[3][3] == 0


def test_filter_on_top(A):
    rng = np.random.default_rng(31)
    masks = [rng.random(s.n_docs) < 0.5 for s in A.segs]
    fid = A.ix.add_filter(masks)
    try:
        qf = np.where(np.arange(16) % 2 == 0, fid, -1).astype(np.int32)
        got = A.check(A.qs, kinds_batch(A), 257, "filter on top", q_filter=qf, filters={fid: masks})
        plain = A.check(A.qs, kinds_batch(A), 257, "no filter")
        assert got[3][12] < plain[3][12] and got[3][0] < plain[3][0] and np.array_equal(got[3][1::2], plain[3][1::2])
        assert plain[3].max() < 257  # (no count is capped at k: the comparisons above are of whole result sets)
    finally:
        A.ix.remove_filter(fid)


def test_field_sort_with_matched_counts(A):
    rng = np.random.default_rng(41)
    vals = [[[int(rng.integers(0, 8))] for _ in range(s.n_docs)] for s in A.segs]
    fields = {"low": (vals, False)}
    fid = A.ix.add_sort_field(vals, np.int64)
    try:
        queries = kinds_batch(A)
        cl = B.clauses_of(queries, 2)
        k_all = sum(s.n_docs for s in A.segs)
        want_all = B.reference(A.oracle, A.segs, *A.qs, k_all, cl)
        for order in ("asc", "desc"):
            sort = [("low", order), ("_score", "desc")]
            for k in (11, 257):
                got = A.ix.search_batch_bool(*A.qs, k, cl, sort=[(fid, order), ("_score", "desc")])
                check_sorted(got, expected_rows(want_all, sort, fields), k, sort, f"sorted {order} k={k}")
        assert got[4][8] == 0 and got[4][15] == 0 and got[4][12] > 0
    finally:
        A.ix.remove_sort_field(fid)


def test_plans_and_the_many_term_kernel(A, oracle):
    """a flat DisMax plan, a two-level plan, and 12 scored lists with min_should 2 (the many-term kernel)"""
    nq = 16
    queries = kinds_batch(A)
    flat = dict(q_leaf=np.tile([0, 0, 1], nq), q_plan=np.full(nq, 1, np.int32), q_tie=np.full(nq, 0.3, F32))
    A.check(A.qs, queries, 257, "flat DisMax", **flat)
    two = dict(q_nleaves=np.full(nq, 3, np.uint32), q_plan=np.zeros(nq, np.int32),
               q_leaf_offsets=(np.arange(nq + 1) * 3).astype(np.uint32),
               leaf_group=np.tile(np.array([0, 0, 1], np.uint32), nq),
               q_group_offsets=(np.arange(nq + 1) * 2).astype(np.uint32),
               group_plan=np.tile(np.array([1, 0], np.int32), nq),
               group_tie=np.tile(np.array([0.3, 0.0], F32), nq))
    A.check(A.qs, queries, 257, "two-level plan", **two)
    rng = np.random.default_rng(51)
    qs = random_queries(rng, 6, 12, 40, n_segs=2, weights=True)
    many = []
    for q in range(6):
        terms = [int(x) for x in qs[1][q * 12:(q + 1) * 12, 0]]
        many.append(([(SHOULD, [t]) for t in terms], 2 if q < 4 else 5))
    many[3] = (many[3][0] + [(MUST_NOT, [int(qs[1][36, 0])])], 2)
    for k in (11, 1025):
        got = A.check(qs, many, k, f"12 lists, min_should 2, k={k}")
    want = oracle.search_batch_min_match(A.segs, *qs, 1025, np.array([2, 2, 2, 0, 5, 5], np.uint32), strategy=oracle.BM25)
    for q in (0, 1, 2, 4, 5):  # the same answer from the oracle's own minimum_should_match
        assert got[3][q] == want[3][q] and np.array_equal(got[0][q], want[0][q])
        assert np.array_equal(got[2][q].view(np.uint32), want[2][q].view(np.uint32))


def test_run_twice_and_batches_in_flight(A, Bw):
    """slg_batch_run twice on one batch gives the same rows (the first pass rewrites what the compaction consumed);
    two batches in flight on their own streams"""
    import torch
    k = 257
    queries = kinds_batch(A)
    cl = B.clauses_of(queries, 2)
    want = B.reference(A.oracle, A.segs, *A.qs, k, cl)
    sd = B.scored_docs(A.segs, A.qs[0], A.qs[1], cl).tolist()
    b = A.ix.prepare(*A.qs, k, clauses=cl)
    for _ in range(2):
        b.run()
        got = b.fetch(want_stats=True)
        same(got, want, "run again")
        assert [int(got[4][q].scored_docs) for q in range(16)] == sd
    b.close()
    T = Bw.T
    qs = csr([[(T["all"], 1.0), (int(t), 0.5)] for t in (3, 5)], 1)
    specs = [B.clauses_of([([(MUST, [T["even"]])], 0), ([(MUST_NOT, [T["d4096"]])], 0)], 1),
             B.clauses_of([([(MUST_NOT, [T["even"]])], 0), ([(SHOULD, [T["d64"]]), (SHOULD, [T["d65"]])], 1)], 1)]
    wants = [B.reference(Bw.oracle, Bw.segs, *qs, k, c) for c in specs]
    streams = [torch.cuda.Stream() for _ in specs]
    batches = [Bw.ix.prepare(*qs, k, clauses=c) for c in specs]
    for bb, s in zip(batches, streams):
        bb.set_stream(s.cuda_stream)
    for _ in range(3):
        for bb in batches:
            bb.run()
    for bb, w in zip(batches, wants):
        same(bb.fetch(), w, "in flight")
        bb.close()


def test_batch_keeps_its_index_state(oracle):
    """a bool batch prepared before slg_index_update_deleted answers against the state it was prepared on"""
    import searchlite_amd as sa
    rng = np.random.default_rng(13)
    segs = [random_segment(rng, 300, 30, 6), random_segment(rng, 200, 30, 6)]
    qs = random_queries(rng, 8, 3, 30, n_segs=2)
    queries = [([(MUST, [int(qs[1][3 * q, 0])]), (MUST_NOT, [int(rng.integers(0, 30))])], 0) for q in range(8)]
    cl = B.clauses_of(queries, 2)
    want_old = B.reference(oracle, [copy.copy(s) for s in segs], *qs, 33, cl)
    with sa.GpuIndex(segs, tuning={"updatable": 1}) as ix:
        b = ix.prepare(*qs, 33, clauses=cl)
        bm = dead_bitmap(rng, 300, 0.3)
        ix.update_deleted(0, bm, 300.0 - float(np.unpackbits(bm, bitorder="little")[:300].sum()))
        b.run()
        same(b.fetch(), want_old, "prepared before the update")
        b.close()
        same(ix.search_batch_bool(*qs, 33, cl), B.reference(oracle, ix.segments, *qs, 33, cl), "prepared after the update")


def test_one_call_form_and_refusals(A):
    """slg_search_batch_bool = prepare + run + fetch; a bool batch does not run sharded; q_min_match > 1 in the
    plans and a clause term id beyond a segment's vocabulary are invalid; the other batch kinds take no clauses"""
    import ctypes as C
    from searchlite_amd import _native as N, searcher
    from searchlite_amd.searcher import bool_spec
    W, k = A, 11
    cl = B.clauses_of(kinds_batch(A), 2)
    spec, keep = bool_spec(cl, 16)
    o, t, w = (np.ascontiguousarray(a) for a in W.qs)
    outs = [np.zeros((16, k), dt) for dt in (np.uint32, np.uint32, F32)] + [np.zeros(16, np.uint32)]
    stats = (N.Stats * 16)()
    N.check(W.ix._lib.slg_search_batch_bool(W.ix._h, 16, o.ctypes.data, t.ctypes.data, w.ctypes.data, None, None, None,
                                            C.addressof(spec), k, 1, *[a.ctypes.data for a in outs],
                                            C.addressof(stats), None))
    same(tuple(outs), B.reference(W.oracle, W.segs, *W.qs, k, cl), "one call")
    assert [int(s.scored_docs) for s in stats] == B.scored_docs(W.segs, o, t, cl).tolist()
    b = W.ix.prepare(*W.qs, k, clauses=cl)
    try:
        group = searcher.ShardGroup(W.ix, 0, 1, searcher.shard_unique_id(), 2)
        try:
            with pytest.raises(N.SlgError) as ei:
                b.run_sharded(group)
            assert ei.value.code == N.ERR_UNSUPPORTED
            with pytest.raises(N.SlgError) as ei:
                b.fetch_sharded()
            assert ei.value.code == N.ERR_UNSUPPORTED
        finally:
            group.close()
        with pytest.raises(N.SlgError):  # score order: no matched counts
            b.run()
            b.matched_counts()
    finally:
        b.close()
    with pytest.raises(N.SlgError) as ei:
        W.ix.prepare(*W.qs, k, clauses=cl, q_min_match=np.full(16, 2, np.uint32))
    assert ei.value.code == N.ERR_INVALID and "q_min_match" in ei.value.msg
    W.ix.prepare(*W.qs, k, clauses=cl, q_min_match=np.ones(16, np.uint32)).close()
    bad = dict(cl, c_terms=np.full_like(cl["c_terms"], 12345))
    with pytest.raises(N.SlgError) as ei:
        W.ix.prepare(*W.qs, k, clauses=bad)
    assert ei.value.code == N.ERR_INVALID and "term id out of range" in ei.value.msg
    for other in (dict(hybrid=True), dict(cursors=[None] * 16)):
        with pytest.raises(N.SlgError) as ei:
            W.ix.prepare(*W.qs, k, clauses=cl, **other)
        assert ei.value.code == N.ERR_UNSUPPORTED


@pytest.mark.parametrize("k", KS)
def test_batches_without_clauses_are_unchanged(oracle, A, k):
    """regression guard: a plain batch on the same queries equals the oracle bit for bit, and a bool batch whose
    queries have no clause table equals it too"""
    want = oracle.search_batch(A.segs, *A.qs, k, strategy=oracle.BM25)
    same(A.ix.search_plan(*A.qs, k), want, f"plain k={k}")
    same(A.ix.search_batch_bool(*A.qs, k, B.clauses_of([([], 0)] * 16, 2)), want, f"empty clause table k={k}")
