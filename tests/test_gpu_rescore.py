"""Query rescore on the device (slg_batch_prepare_rescore, slg_batch_fetch_rescore, slg_search_batch_rescore)
through the C ABI against tests/rescore_ref.py.  Tolerance 0: rows, scores, counts and the three detail arrays
are identical to the reference, bit for bit; rows past the count are zero."""
import numpy as np
import pytest

from tests import rescore_ref as R
from tests.util import _append_lists, assert_same_hits, random_queries, random_segment

pytestmark = pytest.mark.gpu
F32 = np.float32
NO_TERM = 0xFFFFFFFF
KS = (11, 65, 257, 1025)


def windows_of(k):
    return (0, 1, 10, 64, 65, k - 1, k, 5000, 1024)


def same(got, want, what):
    names = ("doc", "seg", "score", "count", "first_score", "rescore_score", "rescored")
    for name, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {name} shape {g.shape} != {w.shape}"
        gb, wb = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == F32 else (g, w)
        if not np.array_equal(gb, wb):
            q, i = (np.argwhere(gb != wb)[0].tolist() + [0])[:2]
            raise AssertionError(f"{what}: {name} differs at query {q} row {i}: {g[q] if g.ndim == 1 else g[q, i]!r} "
                                 f"!= {w[q] if w.ndim == 1 else w[q, i]!r}")
    doc, seg, score, count, first, rsc, flag = got
    for q in range(len(count)):  # rows past the count are zero
        n = int(count[q])
        assert not (doc[q, n:].any() or seg[q, n:].any() or score[q, n:].any() or first[q, n:].any()
                    or rsc[q, n:].any() or flag[q, n:].any()), f"{what}: query {q} has rows past its count"


def dead_bitmap(rng, n, p):
    return np.packbits(rng.random(n) < p, bitorder="little")


class World:
    """segments on the device, first-pass queries, and the oracle's parts of the reference, computed once"""

    def __init__(self, sa, oracle, segs, qs, **plans):
        self.oracle, self.segs, self.qs, self.plans = oracle, segs, qs, plans
        self.ix = sa.GpuIndex(segs)
        self.nq = len(qs[0]) - 1
        self._first, self._maps = {}, {}

    def first(self, k):
        if k not in self._first:
            self._first[k] = R.first_pass(self.oracle, self.segs, *self.qs, k, **self.plans)
        return self._first[k]

    def maps(self, name, rescore):
        if name not in self._maps:
            self._maps[name] = R.rescore_maps(self.oracle, self.segs, rescore)
        return self._maps[name]

    def check(self, k, name, rescore, what):
        got = self.ix.search_rescore(*self.qs, k, rescore, **self.plans)
        want = R.rescore_batch(self.first(k), self.maps(name, rescore), rescore["window"], rescore.get("mode"))
        same(got, want, what)
        return got


def csr(queries, n_segs):
    """[[(term ids per segment or one id, weight)]] -> (q_offsets, q_terms [total, n_segs], q_weights)"""
    offs, terms, ws = [0], [], []
    for q in queries:
        for t, w in q:
            terms.append([t] * n_segs if np.ndim(t) == 0 else list(t))
            ws.append(w)
        offs.append(len(ws))
    return (np.array(offs, np.uint32), np.array(terms, np.uint32).reshape(-1, n_segs), np.array(ws, F32))


@pytest.fixture(scope="module")
def small(oracle):
    """two segments of 300 and 200 docs, vocab 40, tombstones in one, 16 queries: query 7 has no term (no match
    at all), every query matches fewer docs than the larger windows"""
    import searchlite_amd as sa
    rng = np.random.default_rng(7)
    segs = [random_segment(rng, 300, 40, 6), random_segment(rng, 200, 40, 6)]
    segs[1].deleted = dead_bitmap(rng, 200, 0.15)
    o, t, w = random_queries(rng, 16, 3, 40, n_segs=2, weights=True)
    o = o.copy()
    o[8:] -= 3  # query 7 loses its terms
    t, w = np.delete(t, [21, 22, 23], axis=0), np.delete(w, [21, 22, 23])
    W = World(sa, oracle, segs, (o, t, w))
    rq = [[(int(a), float(F32(0.5 + 0.25 * i))) for i, a in enumerate(rng.choice(40, size=2, replace=False))]
          for _ in range(16)]
    rq[3] = []                                 # a rescore query without a term
    rq[5] = [((2, NO_TERM), 1.5), ((NO_TERM, 4), 0.75)]  # terms absent from one segment each
    rq[9] = [(39, 2.0)]                        # a rare term: few rows match
    W.rescore = dict(zip(("q_offsets", "q_terms", "q_weights"), csr(rq, 2)))
    yield W
    W.ix.close()


@pytest.fixture(scope="module")
def big(oracle):
    """one segment of 6000 docs with appended lists: one in every doc (df 6000 > 64 x 64), lists of df 1, 64, 65
    and 4096 whose first and last postings are docs 0 and 5999 (rows of the window), and a list that puts docs
    0, 4321 and 5999 on top of the first pass"""
    import searchlite_amd as sa
    rng = np.random.default_rng(11)
    n, vocab = 6000, 40
    base = random_segment(rng, n, vocab, 6)
    ends = np.array([0, n - 1], np.uint32)

    def with_ends(df):
        inner = rng.choice(np.arange(1, n - 1), size=df - 2, replace=False)
        return np.sort(np.concatenate([ends, inner.astype(np.uint32)]))

    lists = {"all": np.arange(n, dtype=np.uint32), "top": np.array([0, 7, 4321, 5000, n - 1], np.uint32),
             "one": np.array([4321], np.uint32), "d64": with_ends(64), "d65": with_ends(65), "d4096": with_ends(4096),
             "even": np.arange(0, n, 2, dtype=np.uint32)}
    seg = _append_lists(base, [(d, rng.integers(1, 4, size=len(d))) for d in lists.values()])
    T = {name: vocab + i for i, name in enumerate(lists)}
    fq = [[(T["all"], 1.0), (T["top"], 5.0), (int(rng.integers(0, vocab)), 0.5)] for _ in range(6)]
    W = World(sa, oracle, [seg], csr(fq, 1))
    W.T = T
    rq = [[(T["all"], 0.5)], [(T["one"], 3.0)], [(T["d64"], 1.0), (T["d65"], 2.0)],
          [(T["d4096"], 1.0), (T["all"], 0.25), (T["d64"], 4.0)], [(T["d65"], 1.0)], [(T["d4096"], 2.0), (T["one"], 1.0)]]
    W.rescore = dict(zip(("q_offsets", "q_terms", "q_weights"), csr(rq, 1)))
    yield W
    W.ix.close()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("world", ["small", "big"])
def test_k_and_window(request, world, k):
    """every k class and every window of the issue's list, one batch per window (the batch's largest window
    picks the top-k register width); a window that, capped at k, exceeds 1024 is unsupported"""
    from searchlite_amd import _native as N
    W = request.getfixturevalue(world)
    for window in windows_of(k):
        rescore = dict(W.rescore, window=window, mode=R.TOTAL)
        if min(window, k) > N.MAX_RESCORE_WINDOW:
            with pytest.raises(N.SlgError) as ei:
                W.ix.search_rescore(*W.qs, k, rescore)
            assert ei.value.code == N.ERR_UNSUPPORTED
            continue
        got = W.check(k, "base", rescore, f"{world} k={k} window={window}")
        if world == "big" and window >= 10:
            assert got[6][:, :min(window, k)].any()  # (the case rescores something)


def test_first_and_last_postings_are_found(big):
    """docs 0 and 5999 are the first and the last posting of the df 64, 65, 4096 and 6000 lists and rows of the
    window: they are rescored by every query that names such a list"""
    W = big
    doc, seg, score, count, first, rsc, flag = W.check(65, "base", dict(W.rescore, window=64, mode=R.TOTAL), "ends")
    for q in (0, 2, 3, 4, 5):
        for d in (0, 5999):
            i = np.nonzero(doc[q, :64] == d)[0]
            assert len(i) == 1 and flag[q, i[0]] == 1 and rsc[q, i[0]] > 0, (q, d)
    i = np.nonzero(doc[1, :64] == 4321)[0]  # the df 1 list
    assert len(i) == 1 and flag[1, i[0]] == 1 and int(flag[1].sum()) == 1


@pytest.mark.parametrize("world", ["small", "big"])
def test_modes_and_windows_mixed_in_one_batch(request, world):
    W = request.getfixturevalue(world)
    nq = W.nq
    mode = np.arange(nq) % 5
    window = np.array([(0, 1, 10, 64, 65, 200, 256, 5000)[q % 8] for q in range(nq)])
    for k in (65, 257):
        W.check(k, "base", dict(W.rescore, window=window, mode=mode), f"{world} mixed k={k}")
    for m in range(5):
        W.check(65, "base", dict(W.rescore, window=64, mode=m), f"{world} mode {m}")


def test_multiply_by_zero_ties(small, big):
    """weight 0 under multiply: the matched rows become exact 0.0 ties and come out by segment, then doc; the
    others keep their score and lead the window"""
    rs = dict(zip(("q_offsets", "q_terms", "q_weights"), csr([[(0, 0.0)]] * 16, 2)))  # term 0: the commonest
    doc, seg, score, count, first, rsc, flag = small.check(65, "zero", dict(rs, window=64, mode=R.MULTIPLY), "zero small")
    for q in range(16):
        w = min(64, int(count[q]))
        z = np.nonzero(flag[q, :w])[0]
        if len(z) == 0:
            continue
        assert np.all(score[q, z] == 0.0) and z[0] == w - len(z) and np.all(first[q, z] > 0)
        keys = [(int(seg[q, i]), int(doc[q, i])) for i in z]
        assert keys == sorted(keys)
    assert flag.any() and {0, 1} <= set(seg[flag == 1].tolist())
    rs = dict(zip(("q_offsets", "q_terms", "q_weights"), csr([[(big.T["even"], 0.0)]] * 6, 1)))
    doc, seg, score, count, first, rsc, flag = big.check(65, "zero", dict(rs, window=64, mode=R.MULTIPLY), "zero big")
    for q in range(6):
        z = np.nonzero(flag[q, :64])[0]
        assert 16 <= len(z) <= 48 and np.all(doc[q, z] % 2 == 0) and np.all(np.diff(doc[q, z].astype(np.int64)) > 0)
        assert np.array_equal(score[q, :64 - len(z)], first[q, :64 - len(z)])


def test_plans(small):
    """Sum with two terms per leaf; DisMax with tie 0.3 and a leaf absent from one segment; minimum_should_match
    2 over three leaves"""
    rng = np.random.default_rng(3)
    pick = lambda n: [int(x) for x in rng.choice(40, size=n, replace=False)]
    rq = [[(t, float(F32(0.5 + 0.3 * i))) for i, t in enumerate(pick(4))] for _ in range(16)]
    rs = dict(zip(("q_offsets", "q_terms", "q_weights"), csr(rq, 2)), q_leaf=np.tile([0, 0, 1, 1], 16))
    small.check(65, "sum2", dict(rs, window=64, mode=R.TOTAL), "Sum, two terms per leaf")
    rs_d = dict(rs, q_plan=1, q_tie=F32(0.3))
    rs_d["q_terms"] = rs["q_terms"].copy()
    rs_d["q_terms"].reshape(16, 4, 2)[:, 2:, 1] = NO_TERM  # leaf 1 has no term in segment 1
    got = small.check(65, "dismax", dict(rs_d, window=64, mode=R.TOTAL), "DisMax 0.3, leaf absent from a segment")
    assert got[6].any()
    small.check(65, "dismax3", dict(rs_d, q_nleaves=3, window=64, mode=R.MAX), "DisMax with a leaf no term names")
    rq = [[(t, 1.0 + i) for i, t in enumerate(pick(3))] for _ in range(16)]
    rs = dict(zip(("q_offsets", "q_terms", "q_weights"), csr(rq, 2)), q_min_match=2)
    got = small.check(65, "mm2", dict(rs, window=64, mode=R.MULTIPLY), "min_match 2 over three leaves")
    assert 0 < int(got[6].sum()) < int(np.minimum(got[3], 64).sum())  # some rows match, some do not


def test_filtered_and_planned_first_pass(oracle, small):
    """a first pass with a doc filter and a flat score plan; the rescore applies no filter of its own (rows the
    filter passed are rescored although a filter rejects other docs of the rescore lists)"""
    rng = np.random.default_rng(5)
    masks = [rng.random(s.n_docs) < 0.5 for s in small.segs]
    fid = small.ix.add_filter(masks)
    try:
        qf = np.where(np.arange(16) % 2 == 0, fid, -1).astype(np.int32)
        plans = dict(q_leaf=np.tile([0, 0, 1], 15), q_plan=np.full(16, 1, np.int32), q_tie=np.full(16, 0.3, F32))
        k, rescore = 65, dict(small.rescore, window=64, mode=R.TOTAL)
        got = small.ix.search_rescore(*small.qs, k, rescore, q_filter=qf, **plans)
        filters = {fid: masks}
        want = R.reference(oracle, small.segs, *small.qs, k, rescore, q_filter=qf, filters=filters, **plans)
        same(got, want, "filtered DisMax first pass")
        assert got[6].any()
    finally:
        small.ix.remove_filter(fid)


def test_run_twice_and_batches_in_flight(small, big):
    """slg_batch_run twice on one batch gives the same rows (the rescore is not applied twice); two batches in
    flight on their own streams"""
    import torch
    k = 65
    rescore = [dict(W.rescore, window=64, mode=R.MULTIPLY) for W in (small, big)]
    wants = [R.rescore_batch(W.first(k), W.maps("base", rs), 64, R.MULTIPLY) for W, rs in zip((small, big), rescore)]
    b = small.ix.prepare(*small.qs, k, rescore=rescore[0])
    for _ in range(2):
        b.run()
        same(b.fetch() + b.rescore_details(), wants[0], "run again")
    b.close()
    pairs = [(big, rescore[1], wants[1]), (big, dict(rescore[1], mode=R.TOTAL), None)]
    pairs[1] = (big, pairs[1][1], R.rescore_batch(big.first(k), big.maps("base", pairs[1][1]), 64, R.TOTAL))
    streams = [torch.cuda.Stream() for _ in pairs]
    batches = [W.ix.prepare(*W.qs, k, rescore=rs) for W, rs, _ in pairs]
    for bb, s in zip(batches, streams):
        bb.set_stream(s.cuda_stream)
    for _ in range(3):
        for bb in batches:
            bb.run()
    for bb, (_, _, want) in zip(batches, pairs):
        same(bb.fetch() + bb.rescore_details(), want, "in flight")
        bb.close()


def test_batch_keeps_its_index_state(oracle):
    """a rescore batch prepared before slg_index_update_deleted answers against the state it was prepared on"""
    import searchlite_amd as sa
    rng = np.random.default_rng(13)
    segs = [random_segment(rng, 300, 30, 6), random_segment(rng, 200, 30, 6)]
    qs = random_queries(rng, 8, 3, 30, n_segs=2)
    ro, rt, rw = random_queries(rng, 8, 2, 30, n_segs=2, weights=True)
    rescore = dict(q_offsets=ro, q_terms=rt, q_weights=rw, window=32, mode=R.TOTAL)
    want_old = R.reference(oracle, segs, *qs, 33, rescore)
    with sa.GpuIndex(segs, tuning={"updatable": 1}) as ix:
        b = ix.prepare(*qs, 33, rescore=rescore)
        bm = dead_bitmap(rng, 300, 0.3)
        ix.update_deleted(0, bm, 300.0 - float(np.unpackbits(bm, bitorder="little")[:300].sum()))
        b.run()
        same(b.fetch() + b.rescore_details(), want_old, "prepared before the update")
        b.close()
        want_new = R.reference(oracle, ix.segments, *qs, 33, rescore)
        same(ix.search_rescore(*qs, 33, rescore), want_new, "prepared after the update")


def test_one_call_form_and_wrong_batches(small):
    """slg_search_batch_rescore = prepare + run + fetch; slg_batch_fetch_rescore refuses a batch without rescore
    and one that has not run; a rescore term id beyond a segment's vocabulary is invalid"""
    import ctypes as C
    from searchlite_amd import _native as N
    from searchlite_amd.searcher import rescore_spec
    W, k = small, 65
    rescore = dict(W.rescore, window=64, mode=R.MIN)
    spec, keep = rescore_spec(rescore, W.nq)
    o, t, w = (np.ascontiguousarray(a) for a in W.qs)
    outs = [np.zeros((W.nq, k), dt) for dt in (np.uint32, np.uint32, F32)] + [np.zeros(W.nq, np.uint32)] + \
           [np.zeros((W.nq, k), dt) for dt in (F32, F32, np.uint32)]
    N.check(W.ix._lib.slg_search_batch_rescore(W.ix._h, W.nq, o.ctypes.data, t.ctypes.data, w.ctypes.data, None, None,
                                               C.addressof(spec), k, 1, *[a.ctypes.data for a in outs]))
    same(tuple(outs), R.rescore_batch(W.first(k), W.maps("base", rescore), 64, R.MIN), "one call")
    plain = W.ix.prepare(*W.qs, k)
    plain.run()
    assert W.ix._lib.slg_batch_fetch_rescore(plain._h, None, None, None) == N.ERR_INVALID
    assert b"not a rescore batch" in W.ix._lib.slg_last_error()
    plain.close()
    b = W.ix.prepare(*W.qs, k, rescore=rescore)
    assert W.ix._lib.slg_batch_fetch_rescore(b._h, None, None, None) == N.ERR_INVALID
    assert b"has not run" in W.ix._lib.slg_last_error()
    b.close()
    bad = dict(rescore, q_terms=np.full_like(rescore["q_terms"], 12345))
    with pytest.raises(N.SlgError) as ei:
        W.ix.prepare(*W.qs, k, rescore=bad)
    assert ei.value.code == N.ERR_INVALID and "term id out of range" in ei.value.msg


@pytest.mark.parametrize("k", KS)
def test_batches_without_rescore_are_unchanged(oracle, small, big, k):
    """regression guard: a batch without rescore on the same queries equals the oracle bit for bit"""
    for W in (small, big):
        assert_same_hits(W.ix.search_plan(*W.qs, k), W.first(k), 0.0, f"no rescore k={k}")
