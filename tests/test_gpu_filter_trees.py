"""Filter trees built on the device (slg_index_add_filter_trees, slg_index_fetch_filter) through the C ABI against
tests/filter_ref.py.  The rule throughout is equality, tolerance 0 (everything is comparisons and bit operations):

  * fetch_filter of every tree equals filter_ref & ~deleted, bit for bit, for every segment;
  * a search with the tree's id returns rows bit-identical to the same search with the id of
    add_filter(reference mask) (`twin`).

The world is the smallest at which the kernel can go wrong: segments of 1, 31, 32, 33, 63, 64, 65 and 257 docs in one
index (a word edge, a wave edge, the guarded second word of a wave, a block edge), some docs tombstoned, among them
the last doc of three segments; columns of every stored shape; keyword dictionaries of 1, 32, 33 and 70 keys (the
edges of the bit set's words)."""
import copy

import numpy as np
import pytest

from tests import filter_ref as FR
from tests.test_gpu_bool import same
from tests.util import random_queries, random_segment

pytestmark = pytest.mark.gpu
SIZES = (1, 31, 32, 33, 63, 64, 65, 257)
VOCAB = 24
KW, F64, I64, FID, AND, OR, NOT = range(7)
I64_MIN, I64_MAX, TWO53 = -2**63, 2**63 - 1, 2**53
INF = float("inf")

kw = lambda field, begin=0, n=0: dict(kind=KW, field=field, ord_begin=begin, n_ords_in=n)
f64 = lambda field, lo, hi: dict(kind=F64, field=field, lo_f=lo, hi_f=hi)
i64 = lambda field, lo, hi: dict(kind=I64, field=field, lo_i=lo, hi_i=hi)
fid = lambda f: dict(kind=FID, filter_id=f)
AND_ = lambda n: dict(kind=AND, arity=n)
OR_ = lambda n: dict(kind=OR, arity=n)
NOT_ = dict(kind=NOT)


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return sa


def tombstoned(seg, dead):
    s = copy.copy(seg)
    s.deleted = np.packbits(dead, bitorder="little") if dead.any() else None
    s.docs = float(seg.n_docs - int(dead.sum()))
    return s


class World:
    """segments, an index over them, the registered columns by name (filter_ref's field dicts) and the tombstones"""

    def __init__(self, sa, sizes, seed, dead_last=(33, 65, 257), p_dead=0.15):
        self.rng = rng = np.random.default_rng(seed)
        self.dead = []
        segs = []
        for n in sizes:
            dead = rng.random(n) < (p_dead if n > 1 else 0.0)
            if n in dead_last:
                dead[-1] = True
            self.dead.append(dead)
            segs.append(tombstoned(random_segment(rng, n, VOCAB, 5), dead))
        self.segs, self.n_segs = segs, len(segs)
        self.ix = sa.GpuIndex(segs)
        self.fields, self.by_id, self.filter_pass = {}, {}, {}

    def add_numeric(self, name, docs, dtype):
        """docs[s]: per doc a list of values, or None (seg_offsets NULL)"""
        per_seg = [None if d is None else [np.asarray(v, dtype) for v in d] for d in docs]
        f = dict(kind="i64" if np.dtype(dtype) == np.int64 else "f64", keys=None, docs=docs,
                 id=self.ix.add_agg_field(per_seg, dtype))
        self.fields[name] = self.by_id[f["id"]] = f
        return f["id"]

    def add_keyword(self, name, docs, n_ords):
        per_seg = [None if d is None else [np.asarray(v, np.uint32) for v in d] for d in docs]
        f = dict(kind="keyword", keys=[f"{name}-{o}" for o in range(n_ords)], docs=docs,
                 id=self.ix.add_agg_keyword_field(per_seg, n_ords))
        self.fields[name] = self.by_id[f["id"]] = f
        return f["id"]

    def add_mask_filter(self, masks):
        """a host bitmap filter -> its id; a FILTER_ID leaf reads its pass bits: mask & alive"""
        f = self.ix.add_filter(masks)
        self.filter_pass[f] = [np.asarray(m, bool) & ~self.dead[s] for s, m in enumerate(masks)]
        return f

    def want(self, tree):
        nodes, ords = tree
        return [FR.eval_program(nodes, ords, self.by_id, self.filter_pass, s, sg.n_docs) & ~self.dead[s]
                for s, sg in enumerate(self.segs)]

    def check(self, trees, what, search=True):
        """register the trees in one call; every bitmap against filter_ref; then one search per tree under its id
        against the same search under the id of add_filter(reference mask); the filters are removed again"""
        ids = self.ix.add_filter_trees(trees)
        assert len(ids) == len(trees) and len(set(ids)) == len(ids)
        wants = [self.want(t) for t in trees]
        for t, (i, want) in enumerate(zip(ids, wants)):
            got = self.ix.fetch_filter(i)
            for s in range(self.n_segs):
                assert got[s].dtype == bool and got[s].shape == want[s].shape
                if not np.array_equal(got[s], want[s]):
                    d = int(np.argwhere(got[s] != want[s])[0, 0])
                    raise AssertionError(f"{what}: tree {t} segment {s} doc {d}: got {got[s][d]}, want {want[s][d]} "
                                         f"(nodes {trees[t][0]})")
        if search:
            for t in range(0, len(trees), 16):  # (the twins take filter slots too)
                part = list(range(t, min(t + 16, len(trees))))
                twins = [self.ix.add_filter(wants[j]) for j in part]
                qs = random_queries(np.random.default_rng(t), len(part), 2, VOCAB, self.n_segs)
                got = self.ix.search_batch(*qs, 600, q_filter=np.array([ids[j] for j in part], np.int32))
                ref = self.ix.search_batch(*qs, 600, q_filter=np.array(twins, np.int32))
                same(got, ref, f"{what}: search under trees {part[0]}..{part[-1]}")
                for j, q in zip(part, range(len(part))):
                    assert int(got[3][q]) <= sum(int(w.sum()) for w in wants[j])
                for tw in twins:
                    self.ix.remove_filter(tw)
        for i in ids:
            self.ix.remove_filter(i)
        return wants


def value_lists(rng, n, counts, draw):
    """per doc a list of counts[d % len(counts)] values"""
    return [[draw() for _ in range(counts[d % len(counts)])] for d in range(n)]


@pytest.fixture(scope="module")
def world(gpu):
    W = World(gpu, SIZES, 20261018)
    rng = W.rng
    halves = lambda: float(rng.integers(-6, 7)) / 2.0
    specials = [float("nan"), INF, -INF, 0.0, -0.0, 1.5, -1.5]
    ints = [-TWO53, -TWO53 + 1, -3, 0, 3, 7, TWO53 - 1, TWO53]
    # an f64 CSR column with docs holding 0, 1, 2 and 5 values
    W.add_numeric("f", [value_lists(rng, n, (0, 1, 2, 5), halves) for n in SIZES], np.float64)
    # an i64 column stored without offsets (every doc exactly one value), values up to +-2^53 themselves
    W.add_numeric("i", [[[ints[int(rng.integers(0, len(ints)))]] for _ in range(n)] for n in SIZES], np.int64)
    # a column whose second segment has seg_offsets NULL
    W.add_numeric("g", [None if s == 1 else value_lists(rng, n, (1, 0, 3), halves) for s, n in enumerate(SIZES)], np.float64)
    # a column holding NaN, +-inf and +-0.0
    W.add_numeric("x", [value_lists(rng, n, (1, 2, 0, 1), lambda: specials[int(rng.integers(0, len(specials)))])
                        for n in SIZES], np.float64)
    for n_ords, counts in ((1, (1, 0)), (32, (1, 1, 0)), (33, (1,)), (70, (0, 1, 3, 2))):  # k70: multi-valued
        W.add_keyword(f"k{n_ords}", [value_lists(rng, n, counts, lambda: int(rng.integers(0, n_ords))) for n in SIZES], n_ords)
    yield W
    W.ix.close()


def F(W, name):
    return W.fields[name]["id"]


def test_every_segment_size_holds_what_the_world_promises(world):
    """the CPU side: the edges the docstring names exist"""
    W = world
    assert [s.n_docs for s in W.segs] == list(SIZES)
    assert all(W.dead[SIZES.index(n)][-1] for n in (33, 65, 257)) and not W.dead[0].any()
    assert sum(int(d.sum()) for d in W.dead) > 10
    assert {len(v) for d in W.fields["f"]["docs"] for v in d} == {0, 1, 2, 5}
    assert all(len(v) == 1 for d in W.fields["i"]["docs"] for v in d) and W.fields["g"]["docs"][1] is None
    flat = [v for d in W.fields["x"]["docs"] for vals in d for v in vals]
    assert any(np.isnan(v) for v in flat) and INF in flat and -INF in flat
    assert any(v == 0 and np.signbit(v) for v in flat) and any(v == 0 and not np.signbit(v) for v in flat)
    assert max(len(v) for d in W.fields["k70"]["docs"] for v in d) == 3
    assert {TWO53, -TWO53} <= {v for d in W.fields["i"]["docs"] for vals in d for v in vals}


def test_range_leaves_over_every_column_shape(world):
    W = world
    f, i, g, x = F(W, "f"), F(W, "i"), F(W, "g"), F(W, "x")
    leaves = [f64(f, 1.5, 1.5), f64(f, -1.0, 2.0), f64(f, 2.0, -1.0), f64(f, -INF, INF), f64(f, INF, INF), f64(f, -INF, -3.0),
              f64(g, 0.0, 0.0), f64(g, -INF, INF), f64(g, 0.5, 3.0),
              f64(x, 0.0, 0.0), f64(x, -0.0, -0.0), f64(x, -0.0, 0.0), f64(x, -INF, INF), f64(x, INF, INF), f64(x, -INF, -INF),
              f64(x, 1.5, INF), f64(x, -INF, -1.5), f64(x, 1e-300, 1.0),
              i64(i, I64_MIN, I64_MAX), i64(i, I64_MAX, I64_MIN), i64(i, 3, 3), i64(i, -3, 7), i64(i, TWO53, I64_MAX),
              i64(i, I64_MIN, -TWO53), i64(i, TWO53 + 1, I64_MAX), i64(i, -TWO53 + 1, TWO53 - 1), i64(i, 4, 6),
              f64(i, -3.5, 3.5), f64(i, float(TWO53), INF)]
    wants = W.check([([n], []) for n in leaves], "range leaves")
    # -0.0 and 0.0 are one value; NaN never passes, so an unbounded range is "has a value that is not NaN"
    assert all(np.array_equal(a, b) for a, b in zip(wants[9], wants[10])) and any(w.any() for w in wants[9])
    assert not any(w.any() for w in wants[2]) and not any(w.any() for w in wants[19]) and not wants[7][1].any()
    W.check([([n, NOT_], []) for n in leaves], "Not(range leaf)")
    W.check([([n, NOT_, NOT_], []) for n in leaves[::3]], "Not(Not(range leaf))", search=False)


def test_keyword_leaves_at_the_bit_set_word_edges(world):
    W = world
    trees = []
    for n_ords in (1, 32, 33, 70):
        k = F(W, f"k{n_ords}")
        every = list(range(n_ords))
        for ords in ([], every, [n_ords - 1], [n_ords - 1] * 3 + [0, 0], every[::2], [31 % n_ords, 32 % n_ords]):
            trees.append(([kw(k, 0, len(ords))], ords))
            trees.append(([kw(k, 2, len(ords)), NOT_], [7, 7] + ords))  # (a range of the tree's ords, not all of it)
    wants = W.check(trees[:64], "keyword leaves")
    assert not any(w.any() for w in wants[0]) and any(w.any() for w in wants[2])
    # the set of every ordinal passes exactly the live docs that have a value
    k70 = W.fields["k70"]["docs"]
    t = trees.index(([kw(F(W, "k70"), 0, 70)], list(range(70))))
    for s in range(W.n_segs):
        assert np.array_equal(wants[t][s], np.array([len(v) > 0 for v in k70[s]]) & ~W.dead[s])


def test_tree_shapes(world):
    W = world
    f, i, x, k70 = F(W, "f"), F(W, "i"), F(W, "x"), F(W, "k70")
    leaf = lambda j: [f64(f, -3.0 + j * 0.5, -1.0 + j * 0.5), i64(i, -3, 3 + j), kw(k70, 0, 4), f64(x, -INF, 0.0)][j % 4]
    ords = [3, 17, 64, 69]
    chain = [leaf(j) for j in range(16)] + [AND_(2) if j % 3 else OR_(2) for j in range(15)]      # the stack reaches 16
    wide = [leaf(j) for j in range(16)] + [AND_(16)]
    wide_or = [leaf(j) for j in range(16)] + [OR_(16)]
    long = [leaf(0)] + [n for j in range(21) for n in (leaf(j + 1), OR_(2) if j % 2 else AND_(2), NOT_)]
    assert len(long) == 64 and len(chain) == 31
    mixed = [leaf(0), leaf(1), AND_(0), OR_(0), OR_(3), NOT_, leaf(2), AND_(3), leaf(3), NOT_, OR_(2)]
    trees = [([leaf(2)], ords), ([leaf(1), NOT_, NOT_], []), (chain, ords), (wide, ords), (wide_or, ords), (long, ords),
             ([AND_(0)], []), ([OR_(0)], []), ([AND_(0), NOT_], []), ([OR_(0), NOT_], []), ([leaf(0), AND_(1)], []),
             ([leaf(0), OR_(1)], []), (mixed, ords)]
    wants = W.check(trees, "tree shapes")
    for s in range(W.n_segs):  # And([]) passes every live doc, Or([]) none
        assert np.array_equal(wants[6][s], ~W.dead[s]) and not wants[7][s].any()
        assert not wants[8][s].any() and np.array_equal(wants[9][s], ~W.dead[s])
    assert any(w.any() for w in wants[2]) and any(w.any() for w in wants[5])


def test_pass_counts_of_a_65_doc_segment(gpu):
    """0, 1, 63, 64 and all docs of a 65-doc segment pass: no word, one bit of the guarded second word, all but
    one bit of the first wave, the whole first wave, everything"""
    W = World(gpu, (65,), 3, dead_last=(), p_dead=0.0)
    try:
        col = W.add_numeric("n", [[[d] for d in range(65)]], np.int64)
        trees = [([i64(col, 100, 200)], []), ([i64(col, 64, 64)], []), ([i64(col, 1, 63)], []), ([i64(col, 0, 63)], []),
                 ([i64(col, 0, 64)], [])]
        assert [int(W.want(t)[0].sum()) for t in trees] == [0, 1, 63, 64, 65]
        W.check(trees, "pass counts")
    finally:
        W.ix.close()


def term_docs(seg, t):
    m = np.zeros(seg.n_docs, bool)
    m[seg.doc_ids[int(seg.term_offsets[t]):int(seg.term_offsets[t + 1])]] = True
    return m


def test_filter_id_composes_host_bitmaps_and_term_filters(world):
    W = world
    rng = np.random.default_rng(11)
    masks = [rng.random(n) < 0.5 for n in SIZES]
    host = W.add_mask_filter(masks)
    terms = W.ix.add_filter_terms(np.array([[2] * W.n_segs, [5] * W.n_segs], np.uint32), pass_if_absent=True)
    W.filter_pass[terms] = [~(term_docs(sg, 2) | term_docs(sg, 5)) & ~W.dead[s] for s, sg in enumerate(W.segs)]
    f = F(W, "f")
    try:
        # fetch_filter works for the old kinds too
        for flt in (host, terms):
            got = W.ix.fetch_filter(flt)
            assert all(np.array_equal(got[s], W.filter_pass[flt][s]) for s in range(W.n_segs))
        trees = [([fid(host)], []), ([fid(host), NOT_], []), ([fid(terms)], []), ([fid(terms), NOT_], []),
                 ([fid(host), fid(terms), OR_(2), f64(f, -1.0, 2.0), AND_(2)], []),
                 ([fid(host), NOT_, fid(terms), NOT_, AND_(2), NOT_], []), ([fid(host), fid(host), NOT_, OR_(2)], [])]
        wants = W.check(trees, "FILTER_ID")
        for s in range(W.n_segs):  # Not over a registered filter passes no deleted doc: the tombstones are OR-ed in last
            assert np.array_equal(wants[1][s], ~masks[s] & ~W.dead[s])
            assert np.array_equal(wants[6][s], ~W.dead[s])
    finally:
        W.ix.remove_filter(host)
        W.ix.remove_filter(terms)
        del W.filter_pass[host], W.filter_pass[terms]


def test_64_trees_in_one_call_and_all_or_nothing(gpu, world):
    W = world
    f, i, k32 = F(W, "f"), F(W, "i"), F(W, "k32")
    trees = [([f64(f, -3.0 + 0.1 * t, 0.1 * t), i64(i, -3, t), OR_(2), kw(k32, 0, 1 + t % 3), NOT_, AND_(2)], [t % 32, 31, 0])
             for t in range(64)]
    base = W.ix.add_filter([None] * W.n_segs)  # slot policy: the lowest free ids, in the order of the trees
    ids = W.ix.add_filter_trees(trees)
    assert ids == list(range(base + 1, base + 65))
    for t in (0, 31, 63):
        got, want = W.ix.fetch_filter(ids[t]), W.want(trees[t])
        assert all(np.array_equal(got[s], want[s]) for s in range(W.n_segs)), t
    for i_ in ids:
        W.ix.remove_filter(i_)
    W.check(trees, "64 trees")
    # freed slots in the middle are taken first
    a = W.ix.add_filter_trees(trees[:3])
    W.ix.remove_filter(a[1])
    b = W.ix.add_filter_trees(trees[3:5])
    assert a == [base + 1, base + 2, base + 3] and b == [base + 2, base + 4]
    for i_ in (a[0], a[2], *b):
        W.ix.remove_filter(i_)
    # the last tree of 64 is invalid against the state: nothing is registered, no id is handed out
    gen = W.ix.generation
    bad = trees[:63] + [([f64(999, 0.0, 1.0)], [])]
    with pytest.raises(gpu.SlgError) as ei:
        W.ix.add_filter_trees(bad)
    assert ei.value.code == -1 and "unknown agg field id 999" in str(ei.value)
    assert W.ix.generation == gen
    with pytest.raises(gpu.SlgError):
        W.ix.fetch_filter(base + 1)
    assert W.ix.add_filter([None] * W.n_segs) == base + 1
    W.ix.remove_filter(base + 1)
    # against the state: the wrong column kind is invalid, an i64 column beyond +-2^53 unsupported
    big = W.add_numeric("big", [[[TWO53 + 2]] * n for n in SIZES], np.int64)
    for tree, code in ((([i64(f, 0, 1)], []), -1), (([kw(f)], []), -1), (([f64(k32, 0.0, 1.0)], []), -1),
                       (([kw(k32, 0, 1)], [32]), -1), (([fid(base + 7)], []), -1), (([i64(big, 0, 1)], []), -4)):
        with pytest.raises(gpu.SlgError) as ei:
            W.ix.add_filter_trees([tree])
        assert ei.value.code == code, (tree, str(ei.value))
    W.check([([f64(big, 0.0, INF)], [])], "f64 range over the column RANGE_I64 refuses", search=False)
    W.ix.remove_filter(base)


# ---- consumers: one small case each, the tree's id against the id of add_filter(reference mask) -------------
@pytest.fixture(scope="module")
def twin(world):
    W = world
    f, i, k70 = F(W, "f"), F(W, "i"), F(W, "k70")
    tree = ([f64(f, -1.0, 2.0), i64(i, -3, TWO53), AND_(2), kw(k70, 0, 30), NOT_, OR_(2)], list(range(0, 60, 2)))
    (tid,) = W.ix.add_filter_trees([tree])
    want = W.want(tree)
    mid = W.ix.add_filter(want)
    n_pass = sum(int(w.sum()) for w in want)
    assert 50 < n_pass < sum(SIZES) - 50
    yield W, tid, mid, want
    W.ix.remove_filter(tid)
    W.ix.remove_filter(mid)


def both(nq, tid, mid):
    return np.full(nq, tid, np.int32), np.full(nq, mid, np.int32)


def test_consumer_few_term_kernel(twin):
    W, tid, mid, _ = twin
    qs = random_queries(np.random.default_rng(1), 6, 2, VOCAB, W.n_segs, weights=True)
    a, b = both(6, tid, mid)
    for k in (11, 300):
        same(W.ix.search_batch(*qs, k, q_filter=a), W.ix.search_batch(*qs, k, q_filter=b), f"few-term k={k}")
    assert W.ix.search_batch(*qs, 11, q_filter=a)[3].sum() > 0


def test_consumer_many_term_kernel(twin):
    W, tid, mid, _ = twin
    qs = random_queries(np.random.default_rng(2), 4, 12, VOCAB, W.n_segs, weights=True)
    a, b = both(4, tid, mid)
    got = W.ix.search_batch(*qs, 11, q_filter=a)
    same(got, W.ix.search_batch(*qs, 11, q_filter=b), "12 lists")
    assert got[3].sum() > 0


def test_consumer_sorted_batch_with_matched_counts(twin):
    W, tid, mid, want = twin
    sf = W.ix.add_sort_field([[[int(d * 7 % 13)] for d in range(n)] for n in SIZES], np.int64)
    qs = random_queries(np.random.default_rng(3), 4, 2, VOCAB, W.n_segs)
    a, b = both(4, tid, mid)
    got = W.ix.search_sorted(*qs, 11, [(sf, "asc"), ("_score", "desc")], q_filter=a)
    ref = W.ix.search_sorted(*qs, 11, [(sf, "asc"), ("_score", "desc")], q_filter=b)
    same(got[:4], ref[:4], "sorted")
    assert np.array_equal(got[4], ref[4]) and got[4].sum() > 0
    W.ix.remove_sort_field(sf)


def test_consumer_aggregation_batch(twin):
    from searchlite_amd import aggs as A
    W, tid, mid, _ = twin
    fields = {"k33": {"id": F(W, "k33"), "keys": W.fields["k33"]["keys"]}, "f": {"id": F(W, "f")}}
    req = {"t": {"type": "terms", "field": "k33", "aggs": {"s": {"type": "stats", "field": "f"}}}}
    qs = random_queries(np.random.default_rng(4), 3, 2, VOCAB, W.n_segs)
    a, b = both(3, tid, mid)
    got = W.ix.search_aggs(*qs, 11, A.agg_spec(req, fields), q_filter=a)
    ref = W.ix.search_aggs(*qs, 11, A.agg_spec(req, fields), q_filter=b)
    same(got[:4], ref[:4], "aggs hits")
    assert np.array_equal(got[4], ref[4]) and len(got[5]) == len(ref[5]) == 2
    for x, y in zip(got[5], ref[5]):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert got[4].sum() > 0


def test_consumer_function_score_weight_under_the_filter(twin):
    W, tid, mid, _ = twin
    qs = random_queries(np.random.default_rng(5), 4, 2, VOCAB, W.n_segs)
    fn = lambda flt: [dict(functions=[dict(kind="weight", weight=3.0, filter=flt)], score_mode="sum", boost_mode="sum")] * 4
    got = W.ix.search_batch_fscore(*qs, 300, fn(tid))
    same(got, W.ix.search_batch_fscore(*qs, 300, fn(mid)), "function filter")
    plain = W.ix.search_batch(*qs, 300)
    assert np.array_equal(got[3], plain[3]) and not np.array_equal(got[2], plain[2])
    a, b = both(4, tid, mid)
    same(W.ix.search_batch_fscore(*qs, 11, fn(mid), q_filter=a), W.ix.search_batch_fscore(*qs, 11, fn(tid), q_filter=b),
         "function filter and query filter")


def test_consumer_vector_only_search(twin):
    W, tid, mid, want = twin
    rng = np.random.default_rng(6)
    vf = W.ix.add_vector_field([(0, np.arange(n, dtype=np.uint32), rng.standard_normal((n, 8)).astype(np.float32))
                                for n in SIZES])
    qv = rng.standard_normal((3, 8)).astype(np.float32)
    a, b = both(3, tid, mid)
    got = W.ix.vector_search([vf], qv, 1.0, 40, 20, q_filter=a)
    ref = W.ix.vector_search([vf], qv, 1.0, 40, 20, q_filter=b)
    for x, y in zip(got, ref):
        assert x.tobytes() == y.tobytes()
    assert (got[4] == 20).all()


def test_consumer_cursor_page(twin):
    W, tid, mid, _ = twin
    qs = random_queries(np.random.default_rng(7), 4, 2, VOCAB, W.n_segs)
    a, b = both(4, tid, mid)
    first = W.ix.search_batch(*qs, 5, q_filter=a)
    assert (first[3] == 5).all()
    cursors = [((float(first[2][q, 4]),), int(first[1][q, 4]), int(first[0][q, 4])) for q in range(4)]
    got = W.ix.search_after(*qs, 7, cursors, q_filter=a)
    ref = W.ix.search_after(*qs, 7, cursors, q_filter=b)
    same(got[:4], ref[:4], "cursor page")
    assert np.array_equal(got[4], ref[4]) and np.array_equal(got[5], ref[5]) and got[3].sum() > 0
    whole = W.ix.search_batch(*qs, 12, q_filter=a)
    for q in range(4):  # the page continues the first one
        n = int(got[3][q])
        assert np.array_equal(whole[0][q, 5:5 + n], got[0][q, :n]) and np.array_equal(whole[1][q, 5:5 + n], got[1][q, :n])


# ---- lifecycle ------------------------------------------------------------------------------------------------
def test_lifecycle_tombstones_removal_and_new_segments(gpu):
    W = World(gpu, (33, 65), 9)
    try:
        vals = [[[int(d % 11)] for d in range(n)] for n in (33, 65)]
        col = W.add_numeric("n", vals, np.int64)
        tree = ([i64(col, 2, 8), NOT_], [])
        qs = random_queries(np.random.default_rng(8), 3, 2, VOCAB, 2)
        (before,) = W.ix.add_filter_trees([tree])
        # new tombstones for segment 1: a tree registered before the update equals one registered after it
        dead = W.dead[1].copy()
        dead[[0, 31, 32, 63]] = True
        W.ix.update_deleted(1, np.packbits(dead, bitorder="little"), float(65 - dead.sum()))
        W.dead[1] = dead
        (after,) = W.ix.add_filter_trees([tree])
        want = W.want(tree)
        for flt in (before, after):
            got = W.ix.fetch_filter(flt)
            assert all(np.array_equal(got[s], want[s]) for s in range(2)), flt
        same(W.ix.search_batch(*qs, 100, q_filter=np.full(3, before, np.int32)),
             W.ix.search_batch(*qs, 100, q_filter=np.full(3, after, np.int32)), "before / after the tombstones")
        # a batch prepared before slg_index_remove_filter still runs
        ref = W.ix.search_batch(*qs, 100, q_filter=np.full(3, after, np.int32))
        b = W.ix.prepare(*qs, 100, q_filter=np.full(3, after, np.int32))
        W.ix.remove_filter(after)
        b.run()
        same(b.fetch(), ref, "prepared before the removal")
        b.close()
        with pytest.raises(gpu.SlgError):
            W.ix.fetch_filter(after)
        # a new segment: the id is unusable until the tree is registered again, as for every filter
        mask_id = W.ix.add_filter(want)
        new = random_segment(np.random.default_rng(10), 64, VOCAB, 5)
        assert W.ix.add_segment(new) == 2
        W.segs.append(new)
        W.n_segs = 3
        W.dead.append(np.zeros(64, bool))
        qs3 = random_queries(np.random.default_rng(8), 3, 2, VOCAB, 3)
        for flt in (before, mask_id):
            with pytest.raises(gpu.SlgError) as ei:
                W.ix.search_batch(*qs3, 100, q_filter=np.full(3, flt, np.int32))
            assert ei.value.code == -1
        with pytest.raises(gpu.SlgError) as ei:  # the column has no data for the new segment either
            W.ix.add_filter_trees([tree])
        assert ei.value.code == -1 and "no column for segment 2" in str(ei.value)
        with pytest.raises(gpu.SlgError) as ei:
            W.ix.add_filter_trees([([fid(before)], [])])
        assert ei.value.code == -1
        col2 = W.add_numeric("n2", vals + [[[int(d % 11)] for d in range(64)]], np.int64)
        tree2 = ([i64(col2, 2, 8), NOT_], [])
        W.check([tree2], "registered again")
        # slg_index_remove_segment treats the filter like any other: the bitmaps of the segments left stay
        (again,) = W.ix.add_filter_trees([tree2])
        want2 = W.want(tree2)
        W.ix.remove_segment(0)
        got = W.ix.fetch_filter(again)
        assert len(got) == 2 and np.array_equal(got[0], want2[1]) and np.array_equal(got[1], want2[2])
    finally:
        W.ix.close()
