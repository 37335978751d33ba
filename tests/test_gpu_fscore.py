"""function_score on the device (slg_batch_prepare_fscore, slg_search_batch_fscore) through the C ABI against
tests/fscore_ref.py.  Tolerance 0: docs, segments, scores (bit patterns), counts, scored_docs and matched counts are
identical to the reference; rows past the count are zero.

How tolerance 0 is reached: the only operations that are not correctly rounded are the f64 ln, log1p, log2 and pow,
whose result is then rounded to f32.  The worlds pick column values so that every such result is `safe`
(fscore_ref.safe: further than 2^-40 relative from an f32 rounding boundary); unsafe draws are replaced on the CPU
(at most 1 % of them), and every check asserts before the device is touched that none is left."""
import copy
import math

import numpy as np
import pytest

from tests import fscore_ref as R
from tests.test_gpu_bool import csr, dead_bitmap, same
from tests.test_gpu_sort import check as check_sorted, part_key
from tests.util import _append_lists, random_queries, random_segment

pytestmark = pytest.mark.gpu
F32 = np.float32
KS = (1, 11, 257, 1025)

W = lambda w, **kw: dict(kind="weight", weight=w, **kw)
FVF = lambda field, **kw: dict(kind="field_value_factor", field=field, **kw)
DECAY = lambda field, **kw: dict(dict(kind="decay", field=field), **kw)
MODIFIERS = ("none", "log", "log1p", "log2p", "sqrt", "reciprocal")
SCORE_MODES = ("sum", "multiply", "max", "min", "avg")
BOOST_MODES = ("multiply", "sum", "replace", "max", "min")


class World:
    """segments, an index over them, registered columns and filters (by name), and the reference's view of both"""

    def __init__(self, sa, oracle, segs, **tuning):
        self.oracle, self.segs, self.n_segs = oracle, segs, len(segs)
        self.ix = sa.GpuIndex(segs, **tuning)
        self.cols = R.Columns(segs)
        self.F, self.flt, self._cands = {}, {}, {}

    def add_field(self, name, per_seg, dtype):
        fid = self.ix.add_agg_field(per_seg, dtype)
        self.F[name] = fid
        self.cols.fields[fid] = (per_seg, np.dtype(dtype))
        return fid

    def add_filter(self, name, masks):
        fid = self.ix.add_filter(masks)
        self.flt[name] = fid
        self.cols.filters[fid] = masks
        return fid

    def cands(self, qs, plans):
        key = (id(qs), tuple(sorted(plans)))
        if key not in self._cands:  # (one exhaustive oracle run per query set, shared by the checks)
            self._cands[key] = (qs, R.all_candidates(self.oracle, self.segs, *qs, **plans))
        return self._cands[key][1]

    def want(self, qs, functions, k, q_filter=None, **plans):
        assert not R.unsafe_draws(functions, self.cols), "a column value is too close to an f32 rounding boundary"
        return R.apply(self.cands(qs, plans), self.segs, functions, self.cols, k, q_filter)

    def check(self, qs, functions, k, what, q_filter=None, **plans):
        """a function_score batch in score order, with stats -> (got, scored_docs, matched)"""
        want, scored, matched, _ = self.want(qs, functions, k, q_filter, **plans)
        got = self.ix.search_batch_fscore(*qs, k, functions, want_stats=True, q_filter=q_filter, **plans)
        same(got[:4], want, what)
        got_sd = [int(got[4][q].scored_docs) for q in range(len(scored))]
        assert got_sd == scored.tolist(), f"{what}: scored_docs {got_sd} != {scored.tolist()}"
        assert [int(got[4][q].candidates_examined) for q in range(len(scored))] == scored.tolist()
        return got, scored, matched


def safe_column(draw, segs, specs, dtype):
    """per segment one value list per doc from draw(); the draws some function of `specs` (functions over field 0)
    turns into an unsafe f64 are drawn again.  -> per_seg, with at most 1 % of the draws replaced"""
    per_seg = [[draw() for _ in range(s.n_docs)] for s in segs]
    total = sum(s.n_docs for s in segs)
    replaced = 0
    for _ in range(20):
        bad = R.unsafe_draws([dict(functions=specs)], R.Columns(segs, {0: (per_seg, np.dtype(dtype))}))
        if not bad:
            break
        for _, s, d in bad:
            per_seg[s][d] = draw()
            replaced += 1
    assert not bad and replaced <= total // 100, (replaced, total)
    return per_seg


# every transcendental function the tests put on the random columns: the columns are made safe for exactly these
POP = [FVF(0, modifier=m, factor=f) for m in ("log", "log1p", "log2p") for f in (1.0, 0.5, 1.5)]
AGE = [DECAY(0, origin=2500.0, scale=700.0, offset=100.0, decay=d, function=fn) for fn in ("exp", "gauss") for d in (0.5, 0.33, 1.0)] + \
      [DECAY(0, origin=0.0, scale=50.0, decay=0.5, function="gauss"), DECAY(0, origin=0.0, scale=422.0, decay=0.5, function="gauss")]
EDGE_VALUES = [0.0, -1.0, float(np.nextafter(-1.0, -2.0)), float(np.nextafter(-1.0, 0.0)), -5.0, float(np.nextafter(0.0, 1.0)),
               float(np.nextafter(0.0, -1.0)), 1e308, -1e308, 4.0, 0.25, 1e-3]


def on(fn, W_, name):
    """the function with its field (written against field 0 above) renamed to the world's column"""
    return dict(fn, field=W_.F[name])


@pytest.fixture(scope="module")
def A(oracle):
    """two segments of 300 and 200 docs, vocab 40, tombstones in both.  Columns: `pop` f64, 0-3 values per doc (the
    first counts; some docs have none); `age` i64, one value per doc (stored without offsets); `half` f64 whose second
    segment has no offsets at all (every doc of it is without a value); `edge` f64 over the branch edges of the
    modifiers.  Filters: `f0`, `f1` (random halves)"""
    import searchlite_amd as sa
    rng = np.random.default_rng(17)
    segs = [random_segment(rng, 300, 40, 6), random_segment(rng, 200, 40, 6)]
    segs[0].deleted = dead_bitmap(rng, 300, 0.1)
    segs[1].deleted = dead_bitmap(rng, 200, 0.15)
    Wd = World(sa, oracle, segs)
    pop = safe_column(lambda: [float(rng.uniform(0.1, 1000.0)) for _ in range(int(rng.integers(0, 4)))], segs, POP, np.float64)
    age = safe_column(lambda: [int(rng.integers(0, 5001))], segs, AGE, np.int64)
    Wd.add_field("pop", pop, np.float64)
    Wd.add_field("age", age, np.int64)
    Wd.add_field("half", [[[float(rng.uniform(1.0, 9.0))] if rng.random() < 0.7 else [] for _ in range(300)], None], np.float64)
    Wd.add_field("edge", [[[EDGE_VALUES[int(rng.integers(0, len(EDGE_VALUES)))]] for _ in range(s.n_docs)] for s in segs], np.float64)
    Wd.add_filter("f0", [rng.random(s.n_docs) < 0.5 for s in segs])
    Wd.add_filter("f1", [rng.random(s.n_docs) < 0.5 for s in segs])
    Wd.rng = rng
    Wd.qs16 = random_queries(rng, 16, 3, 40, n_segs=2, weights=True)
    Wd.qs25 = random_queries(rng, 25, 3, 40, n_segs=2, weights=True)
    yield Wd
    Wd.ix.close()


@pytest.fixture(scope="module")
def Bw(oracle):
    """one segment of 6000 docs with appended lists of 1, 63, 64, 65, 129 and 6000 docs (one slice each but the
    last).  Column `rank` i64: a doc of the 129-list has its rank in the list, every other doc 1000; `parity` f64:
    doc & 1"""
    import searchlite_amd as sa
    rng = np.random.default_rng(23)
    n, vocab = 6000, 40
    base = random_segment(rng, n, vocab, 6)
    ends = np.array([0, 4321, n - 1], np.uint32)

    def with_ends(df):
        inner = rng.choice(np.setdiff1d(np.arange(1, n - 1), ends), size=df - len(ends), replace=False)
        return np.sort(np.concatenate([ends, inner.astype(np.uint32)])).astype(np.uint32)

    lists = {"c1": np.array([4321], np.uint32), "c63": with_ends(63), "c64": with_ends(64), "c65": with_ends(65),
             "c129": with_ends(129), "all": np.arange(n, dtype=np.uint32)}
    seg = _append_lists(base, [(d, rng.integers(1, 4, size=len(d))) for d in lists.values()])
    Wd = World(sa, oracle, [seg])
    Wd.T = {name: vocab + i for i, name in enumerate(lists)}
    rank = np.full(n, 1000, np.int64)
    rank[lists["c129"]] = np.arange(129)
    Wd.add_field("rank", [[[int(v)] for v in rank]], np.int64)
    Wd.add_field("parity", [[[float(d & 1)] for d in range(n)]], np.float64)
    Wd.lists, Wd.rng = lists, rng
    yield Wd
    Wd.ix.close()


def one_term_queries(Wd, names):
    return csr([[(Wd.T[nm], 1.0 + 0.25 * i)] for i, nm in enumerate(names)], 1)


@pytest.mark.parametrize("kernel", ["lean", "full"])
def test_chunk_edges_of_the_compaction(Bw, kernel):
    """regions of 1, 63, 64, 65, 129 candidates (one slice each) left whole, and the 129 left with 0, 1, 63, 64, 65
    survivors by min_score, on both instantiations"""
    scored = ["c1", "c63", "c64", "c65", "c129"] + ["c129"] * 5
    left = [1, 63, 64, 65, 129, 0, 1, 63, 64, 65]
    qs = one_term_queries(Bw, scored)
    if kernel == "lean":  # the value is the rank: ranks >= 129 - m survive
        fn, bound = FVF(Bw.F["rank"]), lambda m: 129.0 - m
    else:                 # log1p(rank) against log1p(rank - 0.5): far from every value
        fn, bound = FVF(Bw.F["rank"], modifier="log1p"), lambda m: float(F32(math.log1p(129.0 - m - 0.5))) if m < 129 else -1.0
    functions = [dict(functions=[fn], boost_mode="replace", min_score=-1.0)] * 5 + \
                [dict(functions=[fn], boost_mode="replace", min_score=bound(m)) for m in left[5:]]
    # on the CPU first: the regions and the survivors are what the case is about
    want, sd, matched, _ = Bw.want(qs, functions, 257)
    assert [len(Bw.lists[nm]) for nm in scored] == [1, 63, 64, 65, 129, 129, 129, 129, 129, 129]
    assert sd.tolist() == left and matched.tolist() == left
    b = Bw.ix.prepare(*qs, 11, fscore=functions)
    info = b.info()
    b.close()
    assert info["n_slices"] == len(scored) and info["fscore_kernel"] == kernel and info["fscore_queries"] == 10
    for k in (11, 257):
        got, _, _ = Bw.check(qs, functions, k, f"chunk edges {kernel} k={k}")
        assert got[3].tolist() == [min(x, k) for x in left]


@pytest.mark.parametrize("k", KS)
def test_many_slices_all_none_every_other(Bw, k):
    """6000 candidates over several slices: min_score drops all, none, every other one; a negative boost reverses
    the order (the ordered key of negative scores)"""
    T = Bw.T
    qs = csr([[(T["all"], 1.0), (int(t), 0.5)] for t in (3, 5, 7, 9)], 1)
    par = FVF(Bw.F["parity"])
    functions = [dict(functions=[par], boost_mode="replace", min_score=2.0), dict(functions=[par], boost_mode="sum", min_score=-1.0),
                 dict(functions=[par], boost_mode="replace", min_score=0.5), dict(functions=[par], boost_mode="sum", boost=-1.5)]
    b = Bw.ix.prepare(*qs, 11, fscore=functions)
    assert b.info()["n_slices"] > 4 and b.info()["fscore_kernel"] == "lean"
    b.close()
    got, sd, _ = Bw.check(qs, functions, k, f"many slices k={k}")
    assert sd.tolist() == [0, 6000, 3000, 6000] and got[3].tolist() == [0, k, k, k]
    assert np.all(got[0][2, :k] % 2 == 1) and np.all(got[2][3, :k] < 0) and np.all(np.diff(got[2][3, :k]) <= 0)


def test_modifier_branch_edges(A):
    """scaled = 0, -1, just below and above -1, negative, the smallest denormals, +-1e308 under every modifier;
    reciprocal of 0; a product that overflows to inf gives no value"""
    edge = A.F["edge"]
    functions = [dict(functions=[FVF(edge, modifier=m, factor=f)], boost_mode=bm)
                 for m in MODIFIERS for f, bm in ((1.0, "sum"), (10.0, "replace"))] + \
                [dict(functions=[FVF(edge, modifier="reciprocal"), FVF(edge, modifier="sqrt")], score_mode="sum", boost_mode="sum")]
    qs = (A.qs25[0][:len(functions) + 1], A.qs25[1][:3 * len(functions)], A.qs25[2][:3 * len(functions)])
    want, sd, _, _ = A.want(qs, functions, 1025)
    assert np.isinf(want[2]).any() and (sd == A.cands(qs, {})[3]).all()  # (1e308 is inf as f32; nothing is dropped)
    A.check(qs, functions, 1025, "modifier edges")
    b = A.ix.prepare(*qs, 11, fscore=functions)
    assert b.info()["fscore_kernel"] == "full"
    b.close()


def test_decay_edges(A):
    """distance < offset and norm = 0 (value 1.0), gauss underflowing to an f32 denormal and to 0, linear clipped
    at 0, decay = 1, docs without a value, a segment whose column has no offsets at all"""
    age, half = A.F["age"], A.F["half"]
    d = lambda **kw: dict(dict(origin=2500.0, scale=700.0, offset=100.0, decay=0.5, function="exp"), **kw)
    functions = [dict(functions=[DECAY(age, **d(function=fn, decay=dc))], boost_mode=bm)
                 for fn in ("exp", "gauss", "linear") for dc, bm in ((0.5, "multiply"), (0.33, "replace"), (1.0, "sum"))] + \
                [dict(functions=[DECAY(age, origin=0.0, scale=50.0, decay=0.5, function="gauss")], boost_mode="replace"),   # 0
                 dict(functions=[DECAY(age, origin=0.0, scale=422.0, decay=0.5, function="gauss")], boost_mode="replace"),  # denormals
                 dict(functions=[DECAY(age, origin=0.0, scale=100.0, decay=0.25, function="linear")], boost_mode="replace"),
                 dict(functions=[DECAY(half, origin=5.0, scale=2.0, function="linear")], boost_mode="replace"),
                 dict(functions=[FVF(half, missing=3.5, modifier="sqrt"), DECAY(half, origin=5.0, scale=2.0, function="linear")],
                      score_mode="sum", boost_mode="replace", min_score=1.9)]
    qs = tuple(a[:n] for a, n in zip(A.qs16, (len(functions) + 1, 3 * len(functions), 3 * len(functions))))
    want, sd, _, _ = A.want(qs, functions, 1025)  # on the CPU first: the edges are what the case is about
    sc, cnt = want[2], want[3]
    tiny = float(np.finfo(np.float32).tiny)
    assert (sc[9, :cnt[9]] == 0.0).any() and ((sc[10, :cnt[10]] > 0) & (sc[10, :cnt[10]] < tiny)).any()
    assert (sc[11, :cnt[11]] == 0.0).any() and (sc[0, :cnt[0]] > 0).all()
    assert (sc[1, :cnt[1]] == 1.0).any() and (sc[7, :cnt[7]] == 1.0).any()  # norm 0: the value is 1
    assert 0 < sd[13] < A.cands(qs, {})[3][13] and sd[12] == A.cands(qs, {})[3][12]
    A.check(qs, functions, 1025, "decay edges")


def test_score_modes_times_boost_modes(A):
    """all 5 score modes x 5 boost modes on three functions (a weight under a filter, a column, a decay)"""
    fns = [W(1.75, filter=A.flt["f0"]), on(POP[1], A, "pop"), on(AGE[0], A, "age")]
    functions = [dict(functions=fns, score_mode=sm, boost_mode=bm) for sm in SCORE_MODES for bm in BOOST_MODES]
    A.check(A.qs25, functions, 257, "modes")


def test_combine_edges(A):
    """every function filtered out; a base of 0 (weights 0) with and without values; max_boost below and above;
    min_score dropping all and none; a negative boost; no functions but min_score and boost; 8 functions"""
    nobody = A.add_filter("nobody", [np.zeros(s.n_docs, bool) for s in A.segs]) if "nobody" not in A.flt else A.flt["nobody"]
    pop, age, f0 = A.F["pop"], A.F["age"], A.flt["f0"]
    eight = [W(1.25), FVF(pop, modifier="sqrt"), W(0.5, filter=f0), FVF(age, factor=0.001), on(AGE[1], A, "age"),
             FVF(pop, modifier="reciprocal", missing=2.0), W(-0.75, filter=A.flt["f1"]), on(POP[3], A, "pop")]
    functions = [dict(functions=[W(3.0, filter=nobody), FVF(pop, filter=nobody)], boost_mode="replace", min_score=-1e30),
                 dict(functions=[W(3.0, filter=f0)]), dict(functions=[W(3.0, filter=f0)], boost_mode="sum"),
                 dict(functions=[FVF(pop, modifier="sqrt")], max_boost=5.0), dict(functions=[FVF(pop, modifier="sqrt")], max_boost=1e9),
                 dict(functions=[FVF(pop)], boost_mode="replace", min_score=1e9), dict(functions=[FVF(pop)], boost_mode="replace", min_score=-1e9),
                 dict(functions=[FVF(pop, modifier="log1p", factor=0.5)], boost=-2.0),
                 dict(min_score=1.5, boost=3.0), dict(max_boost=1.0, boost=0.5), dict(boost=2.0), None,
                 dict(functions=eight, score_mode="sum", boost_mode="sum"), dict(functions=eight, score_mode="avg", boost_mode="multiply"),
                 dict(functions=eight, score_mode="max", boost_mode="replace", min_score=1.0), dict(functions=eight, score_mode="min", boost_mode="min")]
    want, sd, _, _ = A.want(A.qs16, functions, 257)
    assert sd[5] == 0 and want[3][5] == 0 and want[3][6] > 0 and (want[2][7, :want[3][7]] <= 0).all()
    A.check(A.qs16, functions, 257, "combine edges")
    zero = (A.qs16[0], A.qs16[1], np.zeros_like(A.qs16[2]))  # weights 0: every base score is 0
    want = A.want(zero, functions, 257)[0]
    n1 = int(want[3][1])
    assert n1 > 0 and set(np.unique(want[2][1, :n1]).tolist()) == {0.0, 3.0}  # 1.0 * 3 with a value, the base without
    A.check(zero, functions, 257, "base 0")


@pytest.mark.parametrize("k", KS)
def test_queries_with_and_without_a_spec_in_one_batch(A, k):
    """queries with a spec, without one (None) and with one that has no work mix; the untouched ones are the plain
    batch's rows bit for bit"""
    functions = [dict(functions=[on(POP[4], A, "pop"), on(AGE[3], A, "age")], score_mode="sum", min_score=1.0) if q % 3 == 0
                 else (None if q % 3 == 1 else dict()) for q in range(16)]
    got, _, _ = A.check(A.qs16, functions, k, f"mixed k={k}")
    plain = A.ix.search_plan(*A.qs16, k)
    for q in range(16):
        if q % 3:
            for g, p in zip(got[:3], plain[:3]):
                assert np.array_equal(g[q].view(np.uint32), p[q].view(np.uint32)), f"query {q} was touched"
            assert got[3][q] == plain[3][q]
    b = A.ix.prepare(*A.qs16, k, fscore=functions)
    assert b.info()["fscore_queries"] == 6
    b.close()


def test_nothing_to_do_launches_nothing(A, oracle):
    functions = [None if q % 2 else dict(boost=1.0) for q in range(16)]
    b = A.ix.prepare(*A.qs16, 11, fscore=functions)
    assert b.info()["fscore_kernel"] is None and b.info()["fscore_queries"] == 0
    b.run()
    same(b.fetch(), oracle.search_batch(A.segs, *A.qs16, 11, strategy=oracle.BM25), "no work")
    b.close()


def test_query_filter_on_top_and_function_filters(A):
    f0, f1 = A.flt["f0"], A.flt["f1"]
    qf = np.where(np.arange(16) % 2 == 0, f0, -1).astype(np.int32)
    functions = [dict(functions=[W(2.0, filter=f0 if q % 4 < 2 else f1), on(POP[0], A, "pop")], score_mode="sum",
                      boost_mode="sum", min_score=3.0 if q % 3 == 0 else None) for q in range(16)]
    got, sd, matched = A.check(A.qs16, functions, 257, "filters", q_filter=qf)
    plain, sd2, matched2 = A.check(A.qs16, functions, 257, "no query filter")
    assert sd.tolist() == sd2.tolist() and (matched[0::2] < matched2[0::2]).all() and (matched[1::2] == matched2[1::2]).all()


def test_field_sort_with_matched_counts(A):
    rng = np.random.default_rng(41)
    vals = [[[int(rng.integers(0, 8))] for _ in range(s.n_docs)] for s in A.segs]
    fields = {"low": (vals, False)}
    fid = A.ix.add_sort_field(vals, np.int64)
    try:
        functions = [dict(functions=[on(POP[1], A, "pop"), on(AGE[1], A, "age")], score_mode="multiply", boost_mode="sum",
                          min_score=(2.0 if q % 2 else None), boost=(-1.0 if q % 5 == 0 else 1.0)) for q in range(16)]
        _, _, matched, rows = A.want(A.qs16, functions, 1)
        for order in ("asc", "desc"):
            sort = [("low", order), ("_score", "desc")]
            want = [sorted(hits, key=lambda h: tuple(part_key(p, o, h[0], h[1], h[2], fields) for p, o in sort) + (h[0], h[1]))
                    for hits in rows]
            for k in (11, 257):
                got = A.ix.search_batch_fscore(*A.qs16, k, functions, sort=[(fid, order), ("_score", "desc")])
                check_sorted(got, want, k, sort, f"sorted {order} k={k}")
                assert got[4].tolist() == matched.tolist()
    finally:
        A.ix.remove_sort_field(fid)


def test_plans_and_the_many_term_kernel(A):
    """a flat DisMax plan, a two-level plan, and 12 scored lists (the many-term kernel)"""
    nq = 16
    functions = [dict(functions=[on(POP[2], A, "pop"), W(0.5, filter=A.flt["f1"])], score_mode="max", boost_mode="multiply",
                      min_score=(1.0 if q % 2 else None)) for q in range(nq)]
    flat = dict(q_leaf=np.tile([0, 0, 1], nq), q_plan=np.full(nq, 1, np.int32), q_tie=np.full(nq, 0.3, F32))
    A.check(A.qs16, functions, 257, "flat DisMax", **flat)
    two = dict(q_nleaves=np.full(nq, 3, np.uint32), q_plan=np.zeros(nq, np.int32),
               q_leaf_offsets=(np.arange(nq + 1) * 3).astype(np.uint32), leaf_group=np.tile(np.array([0, 0, 1], np.uint32), nq),
               q_group_offsets=(np.arange(nq + 1) * 2).astype(np.uint32), group_plan=np.tile(np.array([1, 0], np.int32), nq),
               group_tie=np.tile(np.array([0.3, 0.0], F32), nq))
    A.check(A.qs16, functions, 257, "two-level plan", **two)
    qs12 = random_queries(np.random.default_rng(51), 6, 12, 40, n_segs=2, weights=True)
    for k in (11, 1025):
        A.check(qs12, functions[:6], k, f"12 lists k={k}")


def test_run_twice_and_batches_in_flight(A, Bw):
    """slg_batch_run twice on one batch gives the same rows (the scoring kernel rewrites the regions the stage
    consumed); two batches in flight on their own streams"""
    import torch
    k = 257
    functions = [dict(functions=[on(POP[1], A, "pop")], boost_mode="sum", min_score=4.0, boost=0.5)] * 16
    want, sd, _, _ = A.want(A.qs16, functions, k)
    b = A.ix.prepare(*A.qs16, k, fscore=functions)
    for _ in range(2):
        b.run()
        got = b.fetch(want_stats=True)
        same(got[:4], want, "run again")
        assert [int(got[4][q].scored_docs) for q in range(16)] == sd.tolist()
    b.close()
    T = Bw.T
    qs = csr([[(T["all"], 1.0), (int(t), 0.5)] for t in (3, 5)], 1)
    par, rank = FVF(Bw.F["parity"]), FVF(Bw.F["rank"], modifier="sqrt")
    specs = [[dict(functions=[par], boost_mode="replace", min_score=0.5), dict(functions=[rank], boost_mode="sum")],
             [dict(functions=[rank], min_score=30.0), dict(functions=[par], boost_mode="sum", boost=-1.0)]]
    wants = [Bw.want(qs, f, k)[0] for f in specs]
    streams = [torch.cuda.Stream() for _ in specs]
    batches = [Bw.ix.prepare(*qs, k, fscore=f) for f in specs]
    for bb, s in zip(batches, streams):
        bb.set_stream(s.cuda_stream)
    for _ in range(3):
        for bb in batches:
            bb.run()
    for bb, w in zip(batches, wants):
        same(bb.fetch(), w, "in flight")
        bb.close()


def test_batch_keeps_its_index_state(oracle):
    """a batch prepared before slg_index_update_deleted answers against the state it was prepared on"""
    import searchlite_amd as sa
    rng = np.random.default_rng(13)
    segs = [random_segment(rng, 300, 30, 6), random_segment(rng, 200, 30, 6)]
    qs = random_queries(rng, 8, 3, 30, n_segs=2)
    old = [copy.copy(s) for s in segs]
    Wd = World(sa, oracle, segs, tuning={"updatable": 1})
    try:
        fid = Wd.add_field("v", [[[float(rng.integers(1, 100))] for _ in range(s.n_docs)] for s in segs], np.float64)
        functions = [dict(functions=[FVF(fid, modifier="sqrt")], boost_mode="sum", min_score=6.0)] * 8
        want_old = R.apply(R.all_candidates(oracle, old, *qs), old, functions, R.Columns(old, Wd.cols.fields), 33)[0]
        b = Wd.ix.prepare(*qs, 33, fscore=functions)
        bm = dead_bitmap(rng, 300, 0.3)
        Wd.ix.update_deleted(0, bm, 300.0 - float(np.unpackbits(bm, bitorder="little")[:300].sum()))
        b.run()
        same(b.fetch(), want_old, "prepared before the update")
        b.close()
        new = Wd.ix.segments
        want_new = R.apply(R.all_candidates(oracle, new, *qs), new, functions, R.Columns(new, Wd.cols.fields), 33)[0]
        same(Wd.ix.search_batch_fscore(*qs, 33, functions), want_new, "prepared after the update")
    finally:
        Wd.ix.close()


def test_one_call_form_and_refusals(A):
    """slg_search_batch_fscore = prepare + run + fetch; a function_score batch does not run sharded; ids are checked
    against the batch's index state; the other batch kinds take no spec"""
    import ctypes as C
    from searchlite_amd import _native as N, searcher
    k = 11
    functions = [dict(functions=[on(POP[1], A, "pop"), W(2.0, filter=A.flt["f0"])], score_mode="sum", min_score=2.5)] * 16
    spec, keep = searcher.fscore_spec(functions, 16)
    o, t, w = (np.ascontiguousarray(a) for a in A.qs16)
    outs = [np.zeros((16, k), dt) for dt in (np.uint32, np.uint32, F32)] + [np.zeros(16, np.uint32)]
    stats = (N.Stats * 16)()
    N.check(A.ix._lib.slg_search_batch_fscore(A.ix._h, 16, o.ctypes.data, t.ctypes.data, w.ctypes.data, None, None, None,
                                              C.addressof(spec), k, 1, *[a.ctypes.data for a in outs],
                                              C.addressof(stats), None))
    want, sd, _, _ = A.want(A.qs16, functions, k)
    same(tuple(outs), want, "one call")
    assert [int(s.scored_docs) for s in stats] == sd.tolist()
    b = A.ix.prepare(*A.qs16, k, fscore=functions)
    try:
        group = searcher.ShardGroup(A.ix, 0, 1, searcher.shard_unique_id(), 2)
        try:
            for call in (lambda: b.run_sharded(group), b.fetch_sharded):
                with pytest.raises(N.SlgError) as ei:
                    call()
                assert ei.value.code == N.ERR_UNSUPPORTED
        finally:
            group.close()
        with pytest.raises(N.SlgError):  # score order: no matched counts
            b.run()
            b.matched_counts()
    finally:
        b.close()
    kw = A.ix.add_agg_keyword_field([[[0]] * s.n_docs for s in A.segs], 1)
    nonfin = A.ix.add_agg_field([[[math.inf]] * s.n_docs for s in A.segs], np.float64)
    try:
        for fn, code, word in ((FVF(12345), N.ERR_INVALID, "unknown agg field"), (FVF(kw), N.ERR_INVALID, "keyword"),
                               (FVF(nonfin), N.ERR_UNSUPPORTED, "non-finite"), (W(1.0, filter=77), N.ERR_INVALID, "unknown filter"),
                               (W(math.nan), N.ERR_INVALID, "non-finite weight")):
            with pytest.raises(N.SlgError) as ei:
                A.ix.prepare(*A.qs16, k, fscore=[dict(functions=[fn])] * 16)
            assert ei.value.code == code and word in ei.value.msg, fn
        with pytest.raises(N.SlgError) as ei:
            A.ix.prepare(*A.qs16, k, fscore=[dict(functions=[W(1.0)] * 9)] * 16)
        assert ei.value.code == N.ERR_UNSUPPORTED
    finally:
        A.ix.remove_agg_field(kw)
        A.ix.remove_agg_field(nonfin)
    from tests import bool_ref
    for other in (dict(hybrid=True), dict(cursors=[None] * 16), dict(clauses=bool_ref.clauses_of([([], 0)] * 16, 2)),
                  dict(rescore=dict(q_offsets=np.zeros(17, np.uint32), q_terms=np.zeros((0, 2), np.uint32),
                                    q_weights=np.zeros(0, F32), window=4))):
        with pytest.raises(N.SlgError) as ei:
            A.ix.prepare(*A.qs16, k, fscore=functions, **other)
        assert ei.value.code == N.ERR_UNSUPPORTED
