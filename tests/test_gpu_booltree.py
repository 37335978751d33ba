"""Nested boolean matchers on the device (slg_batch_prepare_bool_tree, slg_search_batch_bool_tree) through the C ABI
against tests/booltree_ref.py.  Tolerance 0: docs, segments, scores (bit patterns), counts, scored_docs and matched
counts are identical to the reference; rows past the count are zero.

A registered filter's bitmap carries the tombstones of its segment (reject = deleted | ~filter; a segment given no
mask at registration gets the tombstones alone), so a filter leaf passes `mask & alive`: that is what the worlds
hand the reference for the leaves (it shows in scored_docs only — a tombstoned doc is in no row either way)."""
import copy

import numpy as np
import pytest

from searchlite_amd import booltree as BT
from tests import bool_ref as B
from tests import booltree_ref as R
from tests.test_gpu_bool import KS, csr, dead_bitmap, kinds_batch, same
from tests.test_gpu_sort import check as check_sorted, expected_rows
from tests.util import _append_lists, random_queries, random_segment

pytestmark = pytest.mark.gpu
F32 = np.float32
NO_TERM = 0xFFFFFFFF
MUST, SHOULD, MUST_NOT = B.MUST, B.SHOULD, B.MUST_NOT
T = lambda *ids: {"term": list(ids)}
EDGE_DOCS = (0, 31, 32, 199)  # of the 200-doc segment: word edges of a filter bitmap, and its last doc (200 % 32 != 0)


def alive(seg):
    if seg.deleted is None:
        return np.ones(seg.n_docs, bool)
    return np.unpackbits(np.asarray(seg.deleted, np.uint8), bitorder="little")[:seg.n_docs] == 0


class World:
    def __init__(self, sa, oracle, segs, **tuning):
        self.oracle, self.segs = oracle, segs
        self.ix = sa.GpuIndex(segs, **tuning)
        self.n_segs = len(segs)
        self.filters = {}  # filter id -> [pass bits per segment as a leaf reads them]

    def add_filter(self, masks):
        fid = self.ix.add_filter(masks)
        self.filters[fid] = [alive(s) if m is None else np.asarray(m, bool) & alive(s) for m, s in zip(masks, self.segs)]
        return fid

    def check(self, qs, descs, k, what, **kw):
        """a tree batch of the nested descriptions `descs` over the scored queries qs, with stats -> got"""
        tree = BT.compile_matchers(descs, self.n_segs)
        qf = kw.pop("q_filter", None)
        got = self.ix.search_batch_bool_tree(*qs, k, tree, want_stats=True, q_filter=qf, **kw)
        want = R.reference(self.oracle, self.segs, *qs, k, descs, q_filter=qf, filters=self.filters, **kw)
        same(got, want, what)
        sd = R.scored_docs(self.segs, qs[0], qs[1], descs, self.filters)
        got_sd = [int(got[4][q].scored_docs) for q in range(len(sd))]
        assert got_sd == sd.tolist(), f"{what}: scored_docs {got_sd} != {sd.tolist()}"
        assert [int(got[4][q].candidates_examined) for q in range(len(sd))] == sd.tolist()
        return got


@pytest.fixture(scope="module")
def A(oracle):
    """two segments of 300 and 200 docs, vocab 40, tombstones in both (none on the edge docs); an appended list of
    the edge docs in both segments (term 40); 16 three-term queries"""
    import searchlite_amd as sa
    rng = np.random.default_rng(17)
    segs = [random_segment(rng, 300, 40, 6), random_segment(rng, 200, 40, 6)]
    segs = [_append_lists(s, [(np.array(EDGE_DOCS, np.uint32), np.ones(4, np.uint32))]) for s in segs]
    for s, p in zip(segs, (0.1, 0.15)):
        dead = rng.random(s.n_docs) < p
        dead[list(EDGE_DOCS)] = False
        s.deleted = np.packbits(dead, bitorder="little")
    W = World(sa, oracle, segs)
    W.qs = random_queries(rng, 16, 3, 40, n_segs=2, weights=True)
    W.EDGE = 40
    yield W
    W.ix.close()


def scored_terms(W, q, qs=None):
    o, t, _ = W.qs if qs is None else qs
    return [int(x) for x in t[int(o[q]):int(o[q + 1]), 0]]


@pytest.fixture(scope="module")
def Bw(oracle):
    """one segment of 6000 docs with appended lists.  Clause lists of df 1, 64, 65, 4096 and 6000 whose first and
    last postings (docs 0 and 5999; 4321 for the df 1 list) are candidates; scored lists of 1, 63, 64, 65 and 129
    docs, subsets of the 129 that leave 0, 1, 63, 64, 65 of them, and `alt`: every other doc of the 129"""
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
             "c129": c129, "alt": c129[::2].copy()}
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


def as_tree(groups, min_should):
    """a flat clause table of test_gpu_bool as a one-node tree (None: no clause table)"""
    if not groups:
        return None
    body = {"minimum_should_match": min_should}
    for kind, key in ((MUST, "must"), (SHOULD, "should"), (MUST_NOT, "must_not")):
        body[key] = [T(*terms) for k, terms in groups if k == kind]
    return {"bool": body}


def accepted(W, desc):
    """the matcher's accept mask per segment, on the CPU"""
    return R.nested_masks(W.segs, [desc], W.filters)[0]


def cand(W, qs, q):
    """the candidates of query q per segment: the docs of its scored lists"""
    out = []
    for s, seg in enumerate(W.segs):
        hit = np.zeros(seg.n_docs, bool)
        for i in range(int(qs[0][q]), int(qs[0][q + 1])):
            if int(qs[1][i, s]) != NO_TERM:
                hit[B.postings(seg, int(qs[1][i, s]))] = True
        out.append(hit)
    return out


# ---- equivalence with the flat form ----
@pytest.mark.parametrize("k", KS)
def test_one_node_tree_equals_the_flat_bool_batch(A, k):
    """every kind alone, all kinds together, two-term groups, every min_should, absent terms, no clause table: the
    one-node tree gives what slg_batch_prepare_bool gives for the same clauses, bit for bit"""
    flat = kinds_batch(A)
    got = A.check(A.qs, [as_tree(g, ms) for g, ms in flat], k, f"one-node trees k={k}")
    want = A.ix.search_batch_bool(*A.qs, k, B.clauses_of(flat, 2), want_stats=True)
    same(got[:4], want[:4], f"tree against flat k={k}")
    assert [int(s.scored_docs) for s in got[4]] == [int(s.scored_docs) for s in want[4]]
    assert got[3][8] == 0 and got[3][15] == 0 and got[3][12] > 0


# ---- nested shapes ----
def nested_batch(W, qs):
    st = lambda q: scored_terms(W, q, qs)
    a, b, c = (lambda q: st(q)[0]), (lambda q: st(q)[1]), (lambda q: st(q)[2])
    msm = lambda q, m: {"bool": {"must": [{"bool": {"should": [T(a(q)), T(b(q)), T(c(q))], "minimum_should_match": m}}]}}
    return [
        {"bool": {"must": [{"bool": {"should": [T(a(0)), T(b(0))]}}]}},                       # a bool under must
        {"bool": {"should": [{"bool": {"must": [T(a(1)), T(b(1))]}}, T(7)]}},                 # under should
        {"bool": {"must_not": [{"bool": {"must": [T(a(2))], "must_not": [T(b(2))]}}]}},       # under must_not
        {"bool": {"must": [{"dis_max": [T(a(3)), T(b(3))]}], "must_not": [T(c(3))]}},         # a dis_max child
        {"bool": {"must": [{"query_string": {"terms": [[a(4)], [b(4)]], "not": [[c(4)]]}}]}},  # a query_string child
        {"bool": {"must": ["match_all"], "should": [T(a(5))]}},                               # match_all: everything
        {"bool": {"must_not": ["match_all"]}},                                                # ... and nothing
        {"bool": {"should": [{"dis_max": []}, T(a(7))]}},                                     # an empty dis_max under should
        {"bool": {"must": [T(a(8))], "must_not": [{"dis_max": []}]}},                         # ... under must_not
        {"bool": {"must_not": [{"bool": {"must_not": [T(a(9))]}}]}},                          # double negation
        {"bool": {"must": [{"bool": {"should": [{"bool": {"must_not": [{"dis_max": [T(a(10)), T(5)]}], "must": [T(b(10))]}},
                                                T(c(10))]}}], "must_not": [{"query_string": {"terms": [[3]], "not": [[9]]}}]}},  # depth 4
        msm(11, 0), msm(12, 1), msm(13, 2), msm(14, 4),                                       # min_should at a nested node
        {"bool": {"should": [{"bool": {"must": [T(a(15), 11)]}}]}},                           # a two-term group as a nested leaf
        {"dis_max": [{"bool": {"must": [T(a(16)), T(b(16))]}}, {"query_string": {"not": [[c(16)]]}}]},  # a dis_max root
        T(a(17), b(17)),                                                                      # a matcher that is one term group
    ]


@pytest.mark.parametrize("k", (11, 1025))
def test_nested_shapes(A, k):
    qs = random_queries(np.random.default_rng(3), 18, 3, 40, n_segs=2, weights=True)
    got = A.check(qs, nested_batch(A, qs), k, f"nested shapes k={k}")
    cnt = got[3]
    assert cnt[6] == 0 and cnt[14] == 0 and cnt[5] > 0 and cnt[11] > 0 and cnt[8] > 0 and cnt[10] > 0
    assert cnt[12] >= cnt[13] > 0


# ---- mask edges ----
def chain(n, leaf):
    """n nodes, each holding a leaf and the node before it (odd: should [leaf, below], min_should 1; even: must
    [leaf], must_not [below]); leaf(i): the term of node i's leaf.  The root is node n - 1 and holds leaf 0;
    node 0 holds leaf n - 1"""
    d = {"bool": {"must": [T(leaf(0))]}}
    for i in range(1, n):
        d = {"bool": {"should": [T(leaf(i)), d], "minimum_should_match": 1}} if i % 2 else \
            {"bool": {"must": [T(leaf(i))], "must_not": [d]}}
    return d


def test_mask_edges_32_leaves_64_terms_and_a_32_node_chain(A, Bw):
    # 32 SHOULD leaves of two terms under one node, min_should 8: leaf 31 decides the candidates that hold 7 others
    rng = np.random.default_rng(9)
    pairs = [[int(x) for x in rng.choice(40, size=2, replace=False)] for _ in range(32)]
    wide = lambda last: {"bool": {"should": [T(*p) for p in pairs[:31]] + [T(*last)], "minimum_should_match": 8}}
    tree = BT.compile_matchers([wide(pairs[31])], 2)
    assert int(tree["g_offsets"][1]) == 32 and int(tree["c_offsets"][1]) == 64
    with_, without = accepted(A, wide(pairs[31])), accepted(A, wide([NO_TERM, NO_TERM]))
    cands = cand(A, A.qs, 0)
    assert any(((w != wo) & c).any() for w, wo, c in zip(with_, without, cands))  # on the CPU first: leaf 31 decides
    descs = [wide(pairs[31])] + [None] * 15
    got = A.check(A.qs, descs, 1025, "32 leaves, 64 terms")
    assert 0 < got[3][0] < sum(int(c.sum()) for c in cands)
    # the chain on world B: the odd nodes' leaves `one` (false but for doc 4321), the even nodes' leaves `all`
    # (true), node 0's leaf `even`: every node is the one below it or its negation, so leaf 31 — through node 0
    # (bit 32) and every node up to the root (bit 63) — decides every candidate but 4321, which the root's own
    # leaf (leaf 0) decides
    W, Tm = Bw, Bw.T
    leaf = lambda bottom: (lambda i: Tm[bottom] if i == 0 else (Tm["one"] if i % 2 else Tm["all"]))
    d = chain(32, leaf("even"))
    tree = BT.compile_matchers([d], 1)
    nodes = R.compiled_nodes(tree, 0)
    assert len(nodes) == 32 and int(tree["g_offsets"][1]) == 32
    assert nodes[0] == (1 << 31, 0, 0, 0) and nodes[31][2] == (1 << 0) | (1 << 62)
    acc = accepted(W, d)[0]
    even = np.arange(6000) % 2 == 0
    rest = np.ones(6000, bool)
    rest[4321] = False
    assert np.array_equal(acc[rest], even[rest]) or np.array_equal(acc[rest], ~even[rest])  # leaf 31 decides
    assert acc[4321] and not np.array_equal(accepted(W, chain(32, leaf("none")))[0][rest], acc[rest])
    qs = one_term_queries(W, ["c129", "all"])
    got = W.check(qs, [d, d], 257, "32-node chain")
    in129 = np.isin(W.lists["c129"], np.nonzero(acc)[0])
    assert got[3][0] == int(in129.sum()) and 0 < got[3][0] < 129 and 4321 in got[0][0, :got[3][0]].tolist()


# ---- compaction edges ----
def test_chunk_edges_of_the_compaction(Bw):
    """regions of 1, 63, 64, 65, 129 candidates (one slice each) left with 0, 1, 63, 64, 65, 129 survivors by
    nested trees"""
    W, Tm = Bw, Bw.T
    scored = ["c1", "c63", "c64", "c65", "c129", "c129", "c129", "c129", "c129", "c129", "c129"]
    qs = one_term_queries(W, scored)
    under_must = lambda nm: {"bool": {"must": [{"dis_max": [T(Tm["none"]), T(Tm[nm])]}]}}
    descs = [under_must("all"), {"bool": {"must_not": [{"bool": {"must_not": [T(Tm["all"])]}}]}},
             {"bool": {"should": [{"bool": {"must": [T(Tm["none"])]}}, {"dis_max": [T(Tm["all"])]}]}},
             {"dis_max": [{"bool": {"must": [T(Tm["all"])]}}]}, under_must("all"),
             {"bool": {"must_not": [{"dis_max": [T(Tm["all"])]}]}}, under_must("one"), under_must("k63"),
             {"bool": {"should": [{"query_string": {"terms": [[Tm["k64"]]]}}]}}, under_must("k65"), under_must("none")]
    # on the CPU first: the regions and the survivors are what the case is about
    region = [len(W.lists[nm]) for nm in scored]
    left = R.scored_docs(W.segs, qs[0], qs[1], descs).tolist()
    assert region == [1, 63, 64, 65, 129, 129, 129, 129, 129, 129, 129]
    assert left == [1, 63, 64, 65, 129, 0, 1, 63, 64, 65, 0]
    b = W.ix.prepare(*qs, 11, clause_tree=BT.compile_matchers(descs, 1))
    assert b.info()["n_slices"] == len(scored)  # one slice per query: a region is a slice
    b.close()
    for k in (11, 257):
        got = W.check(qs, descs, k, f"chunk edges k={k}")
        assert got[3].tolist() == [min(x, k) for x in left]


# ---- row steps and early decisions ----
def test_row_steps_and_early_decisions(Bw):
    """rows of 1, 4, 5, 8 and 9 clause terms over the 129 candidates (chunks of 64, 64 and 1).  In each row of more
    than one term the root's MUST_NOT leaf `alt` — every other candidate — comes first and rejects its lanes in the
    first step, while the other lanes are decided only by the LAST should leaf of the nested node (the leaves before
    it hold no candidate).  Then chunks whose every lane is decided after the first step: rejected, and accepted"""
    W, Tm = Bw, Bw.T
    row = lambda n, last: {"bool": {"must_not": [T(Tm["alt"])], "must": [
        {"bool": {"should": [T(Tm["none"])] * (n - 2) + [T(Tm[last])], "minimum_should_match": 1}}]}}
    descs = [{"bool": {"must_not": [{"dis_max": [T(Tm["alt"])]}]}}]  # a row of one term
    descs += [row(n, last) for n in (4, 5, 8, 9) for last in ("all", "k65")]
    descs += [{"bool": {"must_not": [T(Tm["all"])], "should": [T(Tm["d64"])] * 8}},                 # all lanes out at once
              {"bool": {"must": [T(Tm["all"])], "should": [{"dis_max": [T(Tm["d64"])] * 8}]}}]      # ... all in at once
    qs = one_term_queries(W, ["c129"] * len(descs))
    tree = BT.compile_matchers(descs, 1)
    assert np.diff(tree["c_offsets"]).tolist() == [1, 4, 4, 5, 5, 8, 8, 9, 9, 9, 9]
    odd = W.lists["c129"][1::2]
    left = R.scored_docs(W.segs, qs[0], qs[1], descs).tolist()
    k65 = int(np.isin(odd, W.lists["k65"]).sum())
    assert 0 < k65 < 64 and left == [64] + [64, k65] * 4 + [0, 129]
    got = W.check(qs, descs, 257, "row steps")
    assert set(got[0][1, :64].tolist()) == set(odd.tolist())


# ---- binary-search edges under a nested node ----
def test_binary_search_edges_under_nested_nodes(Bw):
    W, Tm = Bw, Bw.T
    names = ["one", "d64", "d65", "d4096", "all"]
    qs = one_term_queries(W, ["c129"] * (2 * len(names)))
    descs = [{"bool": {"should": [{"bool": {"must": [T(Tm[nm])]}}]}} for nm in names] + \
            [{"bool": {"must": [{"bool": {"must_not": [T(Tm[nm])]}}]}} for nm in names]
    got = W.check(qs, descs, 257, "search edges")
    for i, nm in enumerate(names):
        kept, dropped = set(got[0][i, :got[3][i]].tolist()), set(got[0][len(names) + i, :got[3][len(names) + i]].tolist())
        for d in ((4321,) if nm == "one" else (0, 4321, 5999)):
            assert d in kept and d not in dropped, (nm, d)
        assert kept | dropped == set(W.lists["c129"].tolist()) and not (kept & dropped)


# ---- filter leaves ----
def test_filter_leaves(A):
    """a nested bool.filter over a bitmap filter without a bitmap for the second segment; a filter built from a
    filter tree; a filter leaf under must_not; the edge docs of the 200-doc segment on both sides of a filter; a
    q_filter on top"""
    W = A
    rng = np.random.default_rng(31)
    edge = list(EDGE_DOCS)
    m_in = [rng.random(s.n_docs) < 0.5 for s in W.segs]
    m_out = [rng.random(s.n_docs) < 0.5 for s in W.segs]
    for m in m_in:
        m[edge] = True
    for m in m_out:
        m[edge] = False
    f_in, f_out = W.add_filter(m_in), W.add_filter(m_out)
    f_half = W.add_filter([rng.random(300) < 0.5, None])  # no mask for the second segment: passes every live doc there
    vals = [[[int(rng.integers(0, 10))] for _ in range(s.n_docs)] for s in W.segs]
    agg = W.ix.add_agg_field([[np.asarray(v, np.int64) for v in seg] for seg in vals], np.int64)
    (f_tree,) = W.ix.add_filter_trees([([dict(kind=2, field=agg, lo_i=3, hi_i=6)], [])])  # SLG_FILTER_RANGE_I64
    W.filters[f_tree] = [np.array([3 <= v[0] <= 6 for v in seg]) & alive(s) for seg, s in zip(vals, W.segs)]
    f_q = W.add_filter([rng.random(s.n_docs) < 0.6 for s in W.segs])
    try:
        got_tree = W.ix.fetch_filter(f_tree)
        assert all(np.array_equal(g, w) for g, w in zip(got_tree, W.filters[f_tree]))  # what the leaf will read
        qs = csr([[((W.EDGE, W.EDGE), 1.0), (int(t), 0.5)] for t in range(8)], 2)  # the edge docs are candidates
        descs = [
            {"bool": {"must": [{"bool": {"filter": [f_in]}}]}},
            {"bool": {"must": [{"bool": {"filter": [f_out]}}]}},
            {"bool": {"must_not": [{"bool": {"filter": [f_in]}}]}},            # a filter leaf under must_not
            {"bool": {"must_not": [{"bool": {"filter": [f_out]}}]}},
            {"bool": {"should": [{"bool": {"filter": [f_half], "must": [T(1)]}}, {"bool": {"filter": [f_tree]}}]}},
            {"bool": {"filter": [f_tree], "must_not": [{"bool": {"filter": [f_half, f_out]}}]}},
            {"bool": {"filter": [f_half]}},
            None,
        ]
        got = W.check(qs, descs, 1025, "filter leaves")
        rows = lambda q: {(int(s), int(d)) for s, d in zip(got[1][q, :got[3][q]], got[0][q, :got[3][q]])}
        on_edge = {(s, d) for s in (0, 1) for d in edge}
        assert on_edge <= rows(0) and on_edge <= rows(3) and not (on_edge & rows(1)) and not (on_edge & rows(2))
        live = [c & alive(s) for c, s in zip(cand(W, qs, 6), W.segs)]  # f_half: half of segment 0, all of segment 1
        assert sum(1 for s, _ in rows(6) if s == 1) == int(live[1].sum()) and {(1, d) for d in edge} <= rows(6)
        assert 0 < sum(1 for s, _ in rows(6) if s == 0) < int(live[0].sum())
        qf = np.array([f_q, -1] * 4, np.int32)
        top = W.check(qs, descs, 1025, "q_filter on top", q_filter=qf)
        assert top[3][0] < got[3][0] and top[3][4] < got[3][4] and np.array_equal(top[3][1::2], got[3][1::2])
        # an id that names no filter is an error, as in slg_batch_prepare_fscore
        from searchlite_amd import _native as N
        with pytest.raises(N.SlgError) as ei:
            W.ix.prepare(*qs, 11, clause_tree=BT.compile_matchers([{"bool": {"filter": [f_q + 50]}}] + [None] * 7, 2))
        assert ei.value.code == N.ERR_INVALID and "unknown filter id" in ei.value.msg
    finally:
        for f in (f_in, f_out, f_half, f_tree, f_q):
            W.ix.remove_filter(f)
            W.filters.pop(f)
        W.ix.remove_agg_field(agg)


# ---- absent terms ----
def test_absent_terms(A):
    st = lambda q: scored_terms(A, q)
    descs = [
        {"bool": {"must": [{"bool": {"must": [T((st(0)[0], NO_TERM))]}}]}},        # absent from segment 1: no row of it
        {"bool": {"must": [{"dis_max": [T((NO_TERM, st(1)[0]), (st(1)[1], NO_TERM))]}]}},
        {"bool": {"should": [{"bool": {"must": [T((NO_TERM, NO_TERM))]}}, T(st(2)[0])]}},  # absent everywhere under should
        {"bool": {"must": [T(st(3)[0])], "must_not": [{"dis_max": [T((NO_TERM, NO_TERM))]}]}},  # ... under must_not
        {"bool": {"must": [{"bool": {"should": [T((NO_TERM, NO_TERM))]}}]}},       # nothing can hold it
    ] + [None] * 11
    got = A.check(A.qs, descs, 1025, "absent terms")
    cnt = got[3]
    assert cnt[0] > 0 and not (got[1][0, :cnt[0]] == 1).any()
    assert {0, 1} <= set(got[1][1, :cnt[1]].tolist()) and cnt[2] > 0 and cnt[3] > 0 and cnt[4] == 0


# ---- around it ----
def mixed_batch(W):
    """16 queries over world A: nested matchers, one-node matchers and queries without a matcher"""
    o, t, _ = W.qs
    nested = nested_batch(W, (np.arange(19) * 3, np.vstack([t, t[:6]]), None))  # (as queries 16, 17: 0, 1 again)
    return [nested[0], None, nested[2], nested[3], None, nested[4], nested[9], nested[10], nested[12], None,
            nested[13], nested[14], nested[15], as_tree(*kinds_batch(W)[3]), None, nested[6]]


def test_queries_with_and_without_a_matcher(A, oracle):
    descs = mixed_batch(A)
    for k in (11, 257):
        got = A.check(A.qs, descs, k, f"mixed batch k={k}")
    plain = oracle.search_batch(A.segs, *A.qs, 257, strategy=oracle.BM25)
    for q in (1, 4, 9, 14):  # a query without a matcher is left as it is
        assert got[3][q] == plain[3][q] and np.array_equal(got[0][q], plain[0][q])
        assert np.array_equal(got[2][q].view(np.uint32), plain[2][q].view(np.uint32))
    assert got[3][15] == 0


def test_field_sort_with_matched_counts(A):
    rng = np.random.default_rng(41)
    vals = [[[int(rng.integers(0, 8))] for _ in range(s.n_docs)] for s in A.segs]
    fields = {"low": (vals, False)}
    fid = A.ix.add_sort_field(vals, np.int64)
    try:
        descs = mixed_batch(A)
        tree = BT.compile_matchers(descs, 2)
        k_all = sum(s.n_docs for s in A.segs)
        want_all = R.reference(A.oracle, A.segs, *A.qs, k_all, descs)
        for order in ("asc", "desc"):
            sort = [("low", order), ("_score", "desc")]
            for k in (11, 257):
                got = A.ix.search_batch_bool_tree(*A.qs, k, tree, sort=[(fid, order), ("_score", "desc")])
                check_sorted(got, expected_rows(want_all, sort, fields), k, sort, f"sorted {order} k={k}")
        assert got[4][15] == 0 and got[4][1] > 0 and got[4][0] > 0
    finally:
        A.ix.remove_sort_field(fid)


def test_plans_and_the_many_term_kernel(A):
    """a flat DisMax plan, a two-level plan, and 12 scored lists (the many-term kernel)"""
    nq = 16
    descs = mixed_batch(A)
    flat = dict(q_leaf=np.tile([0, 0, 1], nq), q_plan=np.full(nq, 1, np.int32), q_tie=np.full(nq, 0.3, F32))
    A.check(A.qs, descs, 257, "flat DisMax", **flat)
    two = dict(q_nleaves=np.full(nq, 3, np.uint32), q_plan=np.zeros(nq, np.int32),
               q_leaf_offsets=(np.arange(nq + 1) * 3).astype(np.uint32),
               leaf_group=np.tile(np.array([0, 0, 1], np.uint32), nq),
               q_group_offsets=(np.arange(nq + 1) * 2).astype(np.uint32),
               group_plan=np.tile(np.array([1, 0], np.int32), nq),
               group_tie=np.tile(np.array([0.3, 0.0], F32), nq))
    A.check(A.qs, descs, 257, "two-level plan", **two)
    rng = np.random.default_rng(51)
    qs = random_queries(rng, 6, 12, 40, n_segs=2, weights=True)
    many = []
    for q in range(6):
        t = [int(x) for x in qs[1][q * 12:(q + 1) * 12, 0]]
        many.append({"bool": {"must": [{"bool": {"should": [T(x) for x in t[:6]], "minimum_should_match": 2}}],
                              "should": [{"dis_max": [T(t[6]), T(t[7])]}, {"query_string": {"terms": [[t[8]], [t[9]]], "not": [[t[10]]]}}],
                              "must_not": [{"bool": {"must": [T(t[11]), T(t[0])]}}], "minimum_should_match": q % 3}})
    assert np.diff(qs[0]).tolist() == [12] * 6  # (more than the few-term kernel's 8 lists: the many-term kernel)
    for k in (11, 1025):
        got = A.check(qs, many, k, f"12 lists k={k}")
    assert got[3][0] > got[3][2] > 0


def test_run_twice_and_batches_in_flight(A, Bw):
    """slg_batch_run twice on one batch gives the same rows (the first pass rewrites what the compaction consumed);
    two batches in flight on their own streams"""
    import torch
    k = 257
    descs = mixed_batch(A)
    tree = BT.compile_matchers(descs, 2)
    want = R.reference(A.oracle, A.segs, *A.qs, k, descs)
    sd = R.scored_docs(A.segs, A.qs[0], A.qs[1], descs).tolist()
    b = A.ix.prepare(*A.qs, k, clause_tree=tree)
    for _ in range(2):
        b.run()
        got = b.fetch(want_stats=True)
        same(got, want, "run again")
        assert [int(got[4][q].scored_docs) for q in range(16)] == sd
    b.close()
    Tm = Bw.T
    qs = csr([[(Tm["all"], 1.0), (int(t), 0.5)] for t in (3, 5)], 1)
    specs = [[{"bool": {"must": [{"dis_max": [T(Tm["even"])]}]}}, {"bool": {"must_not": [{"bool": {"must": [T(Tm["d4096"])]}}]}}],
             [{"bool": {"must_not": [{"dis_max": [T(Tm["even"])]}]}}, {"bool": {"should": [{"bool": {"should": [T(Tm["d64"]), T(Tm["d65"])]}}]}}]]
    wants = [R.reference(Bw.oracle, Bw.segs, *qs, k, d) for d in specs]
    streams = [torch.cuda.Stream() for _ in specs]
    batches = [Bw.ix.prepare(*qs, k, clause_tree=BT.compile_matchers(d, 1)) for d in specs]
    for bb, s in zip(batches, streams):
        bb.set_stream(s.cuda_stream)
    for _ in range(3):
        for bb in batches:
            bb.run()
    for bb, w in zip(batches, wants):
        same(bb.fetch(), w, "in flight")
        bb.close()


def test_batch_keeps_its_index_state(oracle):
    """a tree batch prepared before slg_index_update_deleted answers against the state it was prepared on"""
    import searchlite_amd as sa
    rng = np.random.default_rng(13)
    segs = [random_segment(rng, 300, 30, 6), random_segment(rng, 200, 30, 6)]
    qs = random_queries(rng, 8, 3, 30, n_segs=2)
    masks = [rng.random(300) < 0.7, rng.random(200) < 0.7]
    with sa.GpuIndex(segs, tuning={"updatable": 1}) as ix:
        fid = ix.add_filter(masks)
        descs = [{"bool": {"must": [{"dis_max": [T(int(qs[1][3 * q, 0])), T(int(qs[1][3 * q + 1, 0]))]}],
                           "must_not": [{"bool": {"must": [T(int(rng.integers(0, 30)))], "filter": [fid]}}]}} for q in range(8)]
        tree = BT.compile_matchers(descs, 2)
        want_old = R.reference(oracle, [copy.copy(s) for s in segs], *qs, 33, descs, filters={fid: masks})
        b = ix.prepare(*qs, 33, clause_tree=tree)
        bm = dead_bitmap(rng, 300, 0.3)
        ix.update_deleted(0, bm, 300.0 - float(np.unpackbits(bm, bitorder="little")[:300].sum()))
        b.run()
        same(b.fetch(), want_old, "prepared before the update")
        b.close()
        same(ix.search_batch_bool_tree(*qs, 33, tree), R.reference(oracle, ix.segments, *qs, 33, descs, filters={fid: masks}),
             "prepared after the update")


def test_one_call_form_and_refusals(A):
    """slg_search_batch_bool_tree = prepare + run + fetch; a tree batch does not run sharded; q_min_match > 1 in the
    plans, a clause term id beyond a segment's vocabulary and the spec's own errors are invalid, its limits
    unsupported; the other batch kinds take no tree"""
    import ctypes as C
    from searchlite_amd import _native as N, searcher
    from searchlite_amd.searcher import bool_tree_spec
    W, k = A, 11
    descs = mixed_batch(A)
    tree = BT.compile_matchers(descs, 2)
    spec, keep = bool_tree_spec(tree, 16)
    o, t, w = (np.ascontiguousarray(a) for a in W.qs)
    outs = [np.zeros((16, k), dt) for dt in (np.uint32, np.uint32, F32)] + [np.zeros(16, np.uint32)]
    stats = (N.Stats * 16)()
    N.check(W.ix._lib.slg_search_batch_bool_tree(W.ix._h, 16, o.ctypes.data, t.ctypes.data, w.ctypes.data, None, None,
                                                 None, C.addressof(spec), k, 1, *[a.ctypes.data for a in outs],
                                                 C.addressof(stats), None))
    same(tuple(outs), R.reference(W.oracle, W.segs, *W.qs, k, descs), "one call")
    assert [int(s.scored_docs) for s in stats] == R.scored_docs(W.segs, o, t, descs).tolist()
    b = W.ix.prepare(*W.qs, k, clause_tree=tree)
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
        W.ix.prepare(*W.qs, k, clause_tree=tree, q_min_match=np.full(16, 2, np.uint32))
    assert ei.value.code == N.ERR_INVALID and "q_min_match" in ei.value.msg
    W.ix.prepare(*W.qs, k, clause_tree=tree, q_min_match=np.ones(16, np.uint32)).close()

    def refused(code, word, **over):
        with pytest.raises(N.SlgError) as ei:
            W.ix.prepare(*W.qs, k, clause_tree=dict(tree, **over))
        assert ei.value.code == code and word in ei.value.msg, ei.value.msg

    refused(N.ERR_INVALID, "term id out of range", c_terms=np.full_like(tree["c_terms"], 12345))
    refused(N.ERR_INVALID, "unknown child kind", e_kind=np.full_like(tree["e_kind"], 7))
    refused(N.ERR_INVALID, "not below its node", e_child=np.full_like(tree["e_child"], 40))
    refused(N.ERR_INVALID, "no node references", e_child=np.zeros_like(tree["e_child"]))
    refused(N.ERR_INVALID, "not monotone", n_offsets=tree["n_offsets"][::-1].copy())
    refused(N.ERR_INVALID, "leaves but no node", n_offsets=np.zeros_like(tree["n_offsets"]))
    for big, word in (({"bool": {"should": [T(g % 40) for g in range(33)]}}, "SLG_MAX_BOOL_TREE_LEAVES"),
                      ({"bool": {"should": ["match_all"] * 32}}, "SLG_MAX_BOOL_TREE_NODES"),
                      ({"bool": {"must": [T(*([3] * 65))]}}, "SLG_MAX_BOOL_TERMS")):
        with pytest.raises(N.SlgError) as ei:
            W.ix.prepare(*W.qs, k, clause_tree=BT.compile_matchers([big] + [None] * 15, 2))
        assert ei.value.code == N.ERR_UNSUPPORTED and word in ei.value.msg
    with pytest.raises(N.SlgError) as ei:
        BT.compile_matchers([{"bool": {"must": [{"phrase": [[1, 2]]}]}}], 2)
    assert ei.value.code == N.ERR_UNSUPPORTED
    for other in (dict(hybrid=True), dict(cursors=[None] * 16), dict(clauses=B.clauses_of([([], 0)] * 16, 2))):
        with pytest.raises(N.SlgError) as ei:
            W.ix.prepare(*W.qs, k, clause_tree=tree, **other)
        assert ei.value.code == N.ERR_UNSUPPORTED


@pytest.mark.parametrize("k", KS)
def test_plain_and_flat_bool_batches_after_a_tree_batch_are_unchanged(oracle, A, k):
    """regression guard: after a tree batch on the same index a plain batch equals the oracle bit for bit, a flat
    bool batch equals its reference, and a tree batch whose queries have no matcher equals the plain batch"""
    A.check(A.qs, mixed_batch(A), k, f"tree batch first k={k}")
    want = oracle.search_batch(A.segs, *A.qs, k, strategy=oracle.BM25)
    same(A.ix.search_plan(*A.qs, k), want, f"plain k={k}")
    flat = kinds_batch(A)
    cl = B.clauses_of(flat, 2)
    same(A.ix.search_batch_bool(*A.qs, k, cl), B.reference(oracle, A.segs, *A.qs, k, cl), f"flat bool k={k}")
    same(A.ix.search_batch_bool_tree(*A.qs, k, BT.compile_matchers([None] * 16, 2)), want, f"no matcher k={k}")
