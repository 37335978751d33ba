"""Cardinality, percentiles and percentile_ranks on the device (slg_index_rank_agg_field + the value nodes of
slg_batch_prepare_aggs).

The aggregated set of a query is what the oracle returns with k >= the number of docs; the expected value tables
are tests/agg_values_ref.py's collectors over that set.  Bar: every u64 cell equal (counts, n); the percentile
cells vals[low] and vals[high] equal under == (as f64: the reference's sort does not order -0.0 and 0.0); the
bucket parents' tables equal to tests/agg_ref.py's; rows bit-identical to the same batch without aggregations;
matched counts equal; two runs of one batch identical.
"""
import copy
import ctypes as C

import numpy as np
import pytest

from tests import agg_ref as R
from tests import agg_values_ref as V
from tests.test_gpu_aggs import docs_of, tombstoned
from tests.util import random_queries, random_segment

pytestmark = pytest.mark.gpu

NO_TERM = 0xFFFFFFFF
KEYS8 = [f"k{i}" for i in range(8)]
KEYSBIG = [f"b{i:04d}" for i in range(2048)]
KEYS_OF = {"kw8": KEYS8, "kwbig": KEYSBIG}
EDGE_R = (1, 31, 32, 33, 64)
F64_COLS = ("zeros", "frac", "p4096", "p4097", "const", "uniq")


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return sa


def make_columns(rng, segs):
    """kw8 / kwbig: keyword fields of 8 / 2048 keys, 0-3 / 0-2 values per doc with repeats; num: i64 in [-50, 50],
    0-2 values; one: i64 in [0, 9], 0-1 value; r<R>: i64 in [0, R), 0-2 values with repeats; zeros: f64 of
    {-0.0, 0.0, 1.5, -2.25}; frac: f64 multiples of 2^-10; p4096 / p4097: exactly that many distinct f64 (multiples
    of 0.5), 1-2 values per doc; const: one value 7.25 per doc; uniq: one value per doc, all distinct"""
    names = ["kw8", "kwbig", "num", "one", "zeros", "frac", "p4096", "p4097", "const", "uniq"] + [f"r{r}" for r in EDGE_R]
    cols = {n: [] for n in names}
    slot = {4096: 0, 4097: 0}
    perm = {r: rng.permutation(r) for r in slot}
    base = 0
    for s in segs:
        n = s.n_docs
        cols["kw8"].append([[KEYS8[j] for j in rng.integers(0, 8, int(rng.integers(0, 4)))] for _ in range(n)])
        cols["kwbig"].append([[KEYSBIG[j] for j in rng.integers(0, 2048, int(rng.integers(0, 3)))] for _ in range(n)])
        cols["num"].append([[int(x) for x in rng.integers(-50, 51, int(rng.integers(0, 3)))] for _ in range(n)])
        cols["one"].append([[int(x) for x in rng.integers(0, 10, int(rng.integers(0, 2)))] for _ in range(n)])
        for r in EDGE_R:
            cols[f"r{r}"].append([[int(x) for x in rng.integers(0, r, int(rng.integers(0, 3)))] for _ in range(n)])
        zs = [-0.0, 0.0, 1.5, -2.25]
        cols["zeros"].append([[zs[j] for j in rng.integers(0, 4, int(rng.integers(0, 3)))] for _ in range(n)])
        cols["frac"].append([[float(x) / 1024.0 for x in rng.integers(-(1 << 20), 1 << 20, int(rng.integers(0, 3)))]
                             for _ in range(n)])
        for r in slot:
            per_doc = []
            for _ in range(n):
                k = int(rng.integers(1, 3))
                per_doc.append([float(perm[r][(slot[r] + j) % r]) * 0.5 for j in range(k)])
                slot[r] += k
            cols[f"p{r}"].append(per_doc)
        cols["const"].append([[7.25] for _ in range(n)])
        cols["uniq"].append([[float(base + d) * 0.25 - 300.0] for d in range(n)])
        base += n
    return cols


def register(ix, cols, names=None, rank=True):
    """-> (the `fields` map of aggs.agg_spec, name -> the distinct count rank_agg_field returned)"""
    fields, ranks = {}, {}
    for name in names or cols:
        if name in KEYS_OF:
            ord_of = {k: i for i, k in enumerate(KEYS_OF[name])}
            per_seg = [[np.array([ord_of[v] for v in d], np.uint32) for d in seg] for seg in cols[name]]
            fields[name] = {"id": ix.add_agg_keyword_field(per_seg, len(ord_of)), "keys": KEYS_OF[name]}
        else:
            fields[name] = {"id": ix.add_agg_field(cols[name], np.float64 if name in F64_COLS else np.int64)}
        if rank:
            ranks[name] = ix.rank_agg_field(fields[name]["id"])
    return fields, ranks


@pytest.fixture(scope="module")
def world(gpu, oracle):
    rng = np.random.default_rng(2026)
    segs = [random_segment(rng, 3000, 60, 25, k1=0.9, b=0.4), random_segment(rng, 1500, 60, 25, k1=0.9, b=0.4),
            random_segment(rng, 800, 60, 25, k1=0.9, b=0.4)]
    segs[0] = tombstoned(segs[0], rng, 0.1)
    segs[2] = tombstoned(segs[2], rng, 0.2)
    offs, terms, w = random_queries(rng, 24, 3, 60, n_segs=3, weights=True)
    terms[-3:, :] = NO_TERM  # the last query matches nothing
    cols = make_columns(rng, segs)
    ix = gpu.GpuIndex(segs)
    fields, ranks = register(ix, cols)
    sort_id = ix.add_sort_field(cols["num"], np.int64)
    k_all = sum(s.n_docs for s in segs)
    all_hits = oracle.search_batch(segs, offs, terms, w, k_all, strategy=oracle.BM25)
    yield dict(ix=ix, segs=segs, offs=offs, terms=terms, w=w, cols=cols, fields=fields, ranks=ranks, k_all=k_all,
               docs=docs_of(all_hits), sort=[(sort_id, "asc"), ("_score", "desc")])
    ix.close()


def as_f64(a):
    return np.ascontiguousarray(a).view(np.float64)


def check_value_tables(plan, request, cols, docs, tables, layout, what="", keys_of=KEYS_OF):
    """the tables of one run against agg_values_ref (value nodes) and agg_ref (the others)"""
    want_layout = V.ref_layout(plan.nodes, cols, keys_of)
    per_q = [V.dense(plan.nodes, want_layout, V.run(request, cols, d), keys_of) for d in docs]
    old = V.strip(request)
    old_nodes = [nd for nd in plan.nodes if nd["body"]["type"] not in V.VALUE_TYPES]
    if old_nodes:
        renum = {i: j for j, i in enumerate(i for i, nd in enumerate(plan.nodes) if nd in old_nodes)}
        flat = [dict(nd, parent=renum.get(nd["parent"], -1)) for nd in old_nodes]
        old_layout = R.ref_layout(flat, cols, keys_of)
        old_q = [R.dense(flat, old_layout, R.run(old, cols, d), keys_of) for d in docs]
    for i, nd in enumerate(plan.nodes):
        gl, wl = layout[i], want_layout[i]
        assert (gl["parent_rows"], gl["rows"]) == (wl["parent_rows"], wl["rows"]), f"{what} node {i}: layout {gl} != {wl}"
        kind = nd["body"]["type"]
        assert gl["is_values"] == (kind in V.VALUE_TYPES)
        if kind not in V.VALUE_TYPES:
            j = old_nodes.index(nd)
            want = np.stack([t[j] for t in old_q])
            if gl["is_stats"]:
                for f in ("count", "min", "max", "sum"):
                    assert np.array_equal(tables[i][f], want[f]), f"{what} node {i}: stats {f} differ"
            else:
                assert np.array_equal(tables[i], want), f"{what} node {i}: counts differ"
            continue
        want = np.stack([t[i] for t in per_q])
        got = tables[i]
        assert got.shape == want.shape and got.dtype == np.uint64, f"{what} node {i}: {got.shape} != {want.shape}"
        if kind != "percentiles":
            assert np.array_equal(got, want), \
                f"{what} node {i} ({kind}): cells differ at {np.argwhere(got != want)[:5].tolist()}"
            continue
        assert np.array_equal(got[..., 0], want[..., 0]), f"{what} node {i}: n differs"
        g, w_ = as_f64(got[..., 1:]), as_f64(want[..., 1:])
        assert np.array_equal(g, w_), f"{what} node {i}: vals[low] / vals[high] differ at {np.argwhere(g != w_)[:5].tolist()}"
    return per_q


def run_check(W, request, sort=None, k=11, docs=None, what="", **kw):
    """one batch with value nodes against the references and against the same batch without aggregations"""
    from searchlite_amd import aggs as A
    ix = W["ix"]
    plan = A.agg_spec(request, W["fields"])
    docs = W["docs"] if docs is None else docs
    doc, seg, score, count, matched, tables, layout = ix.search_aggs(W["offs"], W["terms"], W["w"], k, plan, sort=sort, **kw)
    if sort is None:
        with ix.prepare(W["offs"], W["terms"], W["w"], k, **kw) as b:
            b.run()
            base = b.fetch()
    else:
        base = ix.search_sorted(W["offs"], W["terms"], W["w"], k, sort, **kw)
        assert np.array_equal(matched, base[4]), f"{what}: matched counts changed"
    for name, a, b_ in zip(("doc", "seg", "score", "count"), (doc, seg, score, count), base):
        assert np.array_equal(a.view(np.uint32), b_.view(np.uint32)), f"{what}: {name} rows differ from the plain batch"
    assert matched.tolist() == [len(d) for d in docs], f"{what}: matched"
    per_q = check_value_tables(plan, request, W["cols"], docs, tables, layout, what, W.get("keys_of", KEYS_OF))
    return plan, tables, layout, per_q


# ---- cardinality ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", EDGE_R)
def test_cardinality_at_the_word_edges(gpu, world, r):
    """R = 1, 31, 32, 33, 64 distinct values; a `missing` the dictionary holds (0) and one it does not (1000: one
    rank beyond R, the 32nd / 33rd / 65th bit); docs repeat values"""
    name = f"r{r}"
    assert world["ranks"][name] == r
    assert any(len(d) == 2 and d[0] == d[1] for seg in world["cols"][name] for d in seg), "a doc that repeats a value"
    req = {"a": {"type": "cardinality", "field": name},
           "b": {"type": "cardinality", "field": name, "missing": 0},
           "c": {"type": "cardinality", "field": name, "missing": 1000}}
    _, tables, _, _ = run_check(world, req, what=name)
    assert int(tables[0][:, 0, 0].max()) == r, "some query sees every value"
    assert int(tables[2][:, 0, 0].max()) == r + 1
    run_check(world, req, sort=world["sort"], what=name + " sorted")


def test_cardinality_of_a_keyword_field(gpu, world):
    req = {"a": {"type": "cardinality", "field": "kw8"},
           "own": {"type": "cardinality", "field": "kw8", "missing": "none"},   # missing_ord = n_ords
           "k3": {"type": "cardinality", "field": "kw8", "missing": "k3"},      # a smaller one
           "big": {"type": "cardinality", "field": "kwbig", "missing": "none"}}
    plan, tables, _, _ = run_check(world, req, what="keyword")
    by = {nd["name"]: tables[i][:, 0, 0] for i, nd in enumerate(plan.nodes)}
    assert int(by["own"].max()) == 9 and int(by["a"].max()) == 8 and int(by["big"].max()) > 64


def test_cardinality_tells_the_zeros_apart(gpu, world):
    assert world["ranks"]["zeros"] == 4  # -2.25, -0.0, 0.0, 1.5
    req = {"z": {"type": "cardinality", "field": "zeros"}, "m": {"type": "cardinality", "field": "zeros", "missing": -0.0}}
    _, tables, _, _ = run_check(world, req, what="zeros")
    assert int(tables[1][:, 0, 0].max()) == 4


def test_cardinality_children(gpu, world):
    req = {"t": {"type": "terms", "field": "kw8", "missing": "none",
                 "aggs": {"c": {"type": "cardinality", "field": "num", "missing": 0.5},
                          "k": {"type": "cardinality", "field": "kwbig"},
                          "s": {"type": "stats", "field": "num"}}},
           "h": {"type": "histogram", "field": "num", "interval": 15,
                 "aggs": {"c": {"type": "cardinality", "field": "r33"}}},
           "root": {"type": "cardinality", "field": "frac"}}
    run_check(world, req, what="children")
    run_check(world, req, sort=world["sort"], k=400, what="children sorted k=400")


def test_bitmaps_in_lds_and_in_device_memory_agree(gpu, world):
    """terms(2048 keys) -> cardinality over 64 ranks: 2048 value cells and 2048 x 2 bitmap words are exactly
    SLG_AGG_LDS_BYTES; with the missing key's row (2049) they are just over and live in device memory"""
    from searchlite_amd import _native as N
    child = {"c": {"type": "cardinality", "field": "r64", "missing": 3}}
    under = {"t": {"type": "terms", "field": "kwbig", "aggs": child}}
    over = {"t": {"type": "terms", "field": "kwbig", "missing": "none", "aggs": child}}
    _, t_under, lay_u, _ = run_check(world, under, what="bitmaps in LDS")
    _, t_over, lay_o, _ = run_check(world, over, what="bitmaps in device memory")
    size = lambda lay: 8 * lay[1]["parent_rows"] + 4 * lay[1]["parent_rows"] * 2
    assert size(lay_u) == N.AGG_LDS_BYTES and size(lay_o) > N.AGG_LDS_BYTES
    assert np.array_equal(t_under[1], t_over[1][:, :2048]), "the two homes agree"
    assert t_over[1][:, 2048].any(), "the missing key's bucket has docs"


def test_cardinality_with_a_doc_filter_and_with_k_0(gpu, world, oracle):
    W = world
    rng = np.random.default_rng(8)
    masks = [rng.random(s.n_docs) < 0.5 for s in W["segs"]]
    fid = W["ix"].add_filter(masks)
    nq = len(W["offs"]) - 1
    qf = np.where(np.arange(nq) % 2 == 0, fid, -1).astype(np.int32)
    want = oracle.search_batch_filtered(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], qf, {fid: masks},
                                        strategy=oracle.BM25)
    req = {"c": {"type": "cardinality", "field": "frac"},
           "t": {"type": "terms", "field": "kw8", "aggs": {"c": {"type": "cardinality", "field": "num"}}},
           "p": {"type": "percentiles", "field": "num"},
           "r": {"type": "percentile_ranks", "field": "num", "values": [0]}}
    run_check(W, req, docs=docs_of(want), what="filter", q_filter=qf)
    run_check(W, req, docs=docs_of(want), sort=W["sort"], what="filter sorted", q_filter=qf)
    W["ix"].remove_filter(fid)
    # k = 0: no rows, the same tables (the aggregated set does not depend on k)
    from searchlite_amd import aggs as A
    plan = A.agg_spec(req, W["fields"])
    *_, count, matched, tables, layout = W["ix"].search_aggs(W["offs"], W["terms"], W["w"], 0, plan)
    assert not count.any() and matched.tolist() == [len(d) for d in W["docs"]]
    check_value_tables(plan, req, W["cols"], W["docs"], tables, layout, "k = 0")


# ---- percentile_ranks ----------------------------------------------------------------------------------
def test_percentile_ranks(gpu, world):
    req = {"edges": {"type": "percentile_ranks", "field": "num", "missing": 7,
                     "values": [0, -1000, 1000, -50, 50, 0.5]},   # a value (inclusive), below all, above all
           "sixteen": {"type": "percentile_ranks", "field": "frac", "values": [float(i * 128 - 1024) for i in range(16)]},
           "r": {"type": "range", "field": "num", "ranges": [{"to": 0}, {"from": 0, "to": 25}, {"from": 20}],
                 "aggs": {"pr": {"type": "percentile_ranks", "field": "one", "missing": 4, "values": [4, 8.5]}}}}
    plan, tables, _, _ = run_check(world, req, what="percentile_ranks")
    e = tables[[nd["name"] for nd in plan.nodes].index("edges")][:, 0, :]
    assert not e[:, 2].any() and np.array_equal(e[:, 3], e[:, 0]), "below every value: 0; above every value: n"
    assert (e[:-1, 1] > 0).all() and (e[:-1, 1] < e[:-1, 0]).all(), "a target that is a value counts it (<=)"
    run_check(world, req, sort=world["sort"], what="percentile_ranks sorted")


# ---- percentiles ---------------------------------------------------------------------------------------
def test_percentiles_of_zero_one_and_two_values(gpu, world, oracle):
    """p = 50 over n = 1 and n = 2 values (doc filters that leave one and two of a query's docs) and n = 0"""
    W = world
    d0, d1 = W["docs"][0], W["docs"][1]
    assert len(d0) >= 1 and len(d1) >= 2
    masks = []
    for keep in ([d0[0]], [d1[0], d1[-1]]):
        m = [np.zeros(s.n_docs, bool) for s in W["segs"]]
        for s, d in keep:
            m[s][d] = True
        masks.append(m)
    fids = [W["ix"].add_filter(m) for m in masks]
    nq = len(W["offs"]) - 1
    qf = np.full(nq, -1, np.int32)
    qf[0], qf[1] = fids
    want = docs_of(oracle.search_batch_filtered(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], qf,
                                                dict(zip(fids, masks)), strategy=oracle.BM25))
    assert [len(want[0]), len(want[1]), len(want[-1])] == [1, 2, 0]
    req = {"u": {"type": "percentiles", "field": "uniq", "percents": [50]},      # 5300 ranks: two passes
           "c": {"type": "percentiles", "field": "const", "percents": [50]},     # one rank
           "r": {"type": "percentile_ranks", "field": "uniq", "values": [0.0]}}
    plan, tables, _, _ = run_check(W, req, docs=want, what="n = 0, 1, 2", q_filter=qf)
    u = tables[[nd["name"] for nd in plan.nodes].index("u")][:, 0, :]
    assert u[:, 0].tolist()[:2] == [1, 2] and u[-1].tolist() == [0, 0, 0]
    assert u[0, 1] == u[0, 2] and u[1, 1] != u[1, 2], "n = 1: low == high; n = 2: rank 0.5"
    for f in fids:
        W["ix"].remove_filter(f)


def test_percentiles_edges_sizes_and_missing(gpu, world, oracle):
    """p = 0, 100, out-of-range percents, the defaults; a `missing` with a virtual rank in the middle of the
    dictionary and one the dictionary holds; multi-valued docs; queries on both sides of the reference's 256-value
    limit (a doc filter makes the small ones); all values equal"""
    W = world
    rng = np.random.default_rng(9)
    masks = [rng.random(s.n_docs) < 0.05 for s in W["segs"]]
    fid = W["ix"].add_filter(masks)
    nq = len(W["offs"]) - 1
    qf = np.where(np.arange(nq) % 2 == 1, fid, -1).astype(np.int32)
    want = docs_of(oracle.search_batch_filtered(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], qf, {fid: masks},
                                                strategy=oracle.BM25))
    edges = [0, 100, -5, 250, 50, 33.3]
    req = {"num": {"type": "percentiles", "field": "num", "percents": edges},                       # 101 ranks
           "mid": {"type": "percentiles", "field": "num", "percents": edges, "missing": 0.5},       # virtual rank 51
           "held": {"type": "percentiles", "field": "num", "missing": -50},
           "frac": {"type": "percentiles", "field": "frac", "percents": edges, "missing": 0.0001},  # two passes
           "zeros": {"type": "percentiles", "field": "zeros"},
           "const": {"type": "percentiles", "field": "const", "percents": [0, 50, 100]}}
    plan, tables, _, per_q = run_check(W, req, docs=want, what="percentile edges", q_filter=qf)
    names = [nd["name"] for nd in plan.nodes]
    n = tables[names.index("num")][:, 0, 0]
    assert ((n > 0) & (n <= V.EXACT_LIMIT)).any() and (n > V.EXACT_LIMIT).any(), n.tolist()
    assert any(len(d) == 2 for seg in W["cols"]["num"] for d in seg), "multi-valued docs"
    assert W["ranks"]["num"] == 101 and W["ranks"]["frac"] > 4096
    c = as_f64(tables[names.index("const")][:-1, 0, 1:])
    assert (c == 7.25).all()
    W["ix"].remove_filter(fid)


@pytest.mark.parametrize("r", [4096, 4097])
def test_percentiles_one_pass_and_two(gpu, world, r):
    """4096 ranks: a coarse bin is a rank (one pass); 4097: shift 1, two passes.  A virtual `missing` makes them
    4097 and 4098."""
    name = f"p{r}"
    assert world["ranks"][name] == r
    req = {"d": {"type": "percentiles", "field": name},
           "m": {"type": "percentiles", "field": name, "missing": 1000.25},
           "c": {"type": "cardinality", "field": name}}
    run_check(world, req, what=name)


def test_percentiles_across_coarse_bins(gpu, world):
    """Over 4097 ranks (two ranks per coarse bin): a percent whose low is the last element of a bin and whose high
    is the first of the next one, for query 0; and 16 percents that land in 16 different bins"""
    W = world
    vals = sorted(v for s, d in W["docs"][0] for v in W["cols"]["p4097"][s][d])
    dictionary = sorted({v for seg in W["cols"]["p4097"] for d in seg for v in d})
    assert len(dictionary) == 4097
    bin_of = lambda v: dictionary.index(v) >> 1
    n = len(vals)
    i = next(i for i in range(n // 3, n - 1) if bin_of(vals[i]) != bin_of(vals[i + 1]))
    split = 100.0 * (i + 0.5) / (n - 1)
    _, low, high = V.rank_low_high(n, split)
    assert (low, high) == (i, i + 1) and bin_of(vals[low]) + 1 <= bin_of(vals[high])
    sixteen = [3.0 + 6.0 * j for j in range(16)]
    bins = {bin_of(vals[V.rank_low_high(n, p)[1]]) for p in sixteen}
    assert len(bins) == 16, "16 different coarse bins for query 0"
    req = {"split": {"type": "percentiles", "field": "p4097", "percents": [split, 50]},
           "sixteen": {"type": "percentiles", "field": "p4097", "percents": sixteen}}
    run_check(W, req, what="across bins")
    run_check(W, req, sort=W["sort"], what="across bins sorted")


def test_fine_tables_in_lds_and_in_device_memory(gpu, oracle):
    """540 000 distinct values (90 per doc): 2^20 ranks' worth of shift = 8.  The 7 default percents need 14 x 256
    fine cells (14 KB: LDS), 16 percents 32 x 256 (32 KB: the scratch slice)."""
    from searchlite_amd import _native as N, aggs as A
    rng = np.random.default_rng(77)
    seg = random_segment(rng, 6000, 40, 20, k1=0.9, b=0.4)
    offs, terms, w = random_queries(rng, 4, 3, 40, n_segs=1, weights=True)
    per_doc = 90
    values = rng.permutation(6000 * per_doc).astype(np.float64) * 0.5 - 1000.0
    csr = (np.arange(6001, dtype=np.uint32) * per_doc, values)
    cols = {"big": [[values[d * per_doc:(d + 1) * per_doc].tolist() for d in range(6000)]]}
    docs = docs_of(oracle.search_batch([seg], offs, terms, w, 6000, strategy=oracle.BM25))
    sixteen = [1.0 + 6.5 * j for j in range(16)]
    with gpu.GpuIndex([seg]) as ix:
        fid = ix.add_agg_field([csr], np.float64)
        assert ix.rank_agg_field(fid) == 6000 * per_doc and ix.rank_agg_field(fid) == 6000 * per_doc
        shift = int(np.ceil(np.log2(6000 * per_doc))) - 12
        assert shift == 8 and 4 * (14 << shift) <= N.AGG_PCT_LDS_BYTES < 4 * (32 << shift)
        for name, body in (("fine tables in LDS", {"type": "percentiles", "field": "big"}),
                           ("fine tables in device memory", {"type": "percentiles", "field": "big", "percents": sixteen}),
                           ("with a bitmap beside them", {"type": "percentiles", "field": "big", "percents": sixteen,
                                                          "missing": 0.25})):
            req = {"p": body, "c": {"type": "cardinality", "field": "big"}} if "bitmap" in name else {"p": body}
            plan = A.agg_spec(req, {"big": {"id": fid}})
            *_, matched, tables, layout = ix.search_aggs(offs, terms, w, 11, plan)
            assert matched.tolist() == [len(d) for d in docs]
            check_value_tables(plan, req, cols, docs, tables, layout, name)


# ---- refusals, updates, repeat runs --------------------------------------------------------------------
def test_refusals(gpu, world):
    from searchlite_amd import _native as N, aggs as A
    W = world
    ix = W["ix"]

    def fails(code, request, word, fields=None):
        with pytest.raises(N.SlgError) as ei:
            ix.search_aggs(W["offs"], W["terms"], W["w"], 11, A.agg_spec(request, fields or W["fields"]))
        assert ei.value.code == code and word in str(ei.value), ei.value

    pct = {"type": "percentiles", "field": "num"}
    fails(N.ERR_UNSUPPORTED, {"t": {"type": "terms", "field": "kw8", "aggs": {"p": pct}}}, "root")
    # a numeric field without ranks: cardinality and percentiles name the call that makes them; percentile_ranks
    # needs none
    plain = {"x": {"id": ix.add_agg_field(W["cols"]["num"], np.int64)}}
    fails(N.ERR_INVALID, {"p": {"type": "percentiles", "field": "x"}}, "slg_index_rank_agg_field", plain)
    fails(N.ERR_INVALID, {"c": {"type": "cardinality", "field": "x"}}, "slg_index_rank_agg_field", plain)
    ranks_only = {"r": {"type": "percentile_ranks", "field": "x", "values": [0]}}
    got = ix.search_aggs(W["offs"], W["terms"], W["w"], 11, A.agg_spec(ranks_only, plain))
    check_value_tables(A.agg_spec(ranks_only, plain), ranks_only, {"x": W["cols"]["num"]}, W["docs"], got[5], got[6])
    # the wrong kind of field
    fails(N.ERR_INVALID, {"p": {"type": "percentiles", "field": "kw8"}}, "keyword")
    fails(N.ERR_INVALID, {"r": {"type": "percentile_ranks", "field": "kw8", "values": [1]}}, "keyword")
    # i64 values beyond 2^53 do not rank: two of them became one f64
    big = [[[(1 << 53) + 1] if d == 0 else [d] for d in range(s.n_docs)] for s in W["segs"]]
    bid = ix.add_agg_field(big, np.int64)
    with pytest.raises(N.SlgError) as ei:
        ix.rank_agg_field(bid)
    assert ei.value.code == N.ERR_UNSUPPORTED and "2^53" in str(ei.value)
    nan = [[[float("nan")] if d == 0 else [1.0] for d in range(s.n_docs)] for s in W["segs"]]
    with pytest.raises(N.SlgError) as ei:
        ix.rank_agg_field(ix.add_agg_field(nan, np.float64))
    assert ei.value.code == N.ERR_UNSUPPORTED
    with pytest.raises(N.SlgError) as ei:
        ix.rank_agg_field(12345)
    assert ei.value.code == N.ERR_INVALID
    assert ix.rank_agg_field(W["fields"]["kw8"]["id"]) == 8, "a keyword field's ordinals are its ranks"
    # scratch above the cap: 4097 histogram rows x ceil(4097 / 32) = 129 bitmap words > 2^19
    cap = {"h": {"type": "histogram", "field": "p4097", "interval": 0.5,
                 "aggs": {"c": {"type": "cardinality", "field": "p4097"}}}}
    assert 4097 * 129 > N.MAX_AGG_SCRATCH_WORDS
    fails(N.ERR_UNSUPPORTED, cap, "SLG_MAX_AGG_SCRATCH_WORDS")
    # value cells count towards SLG_MAX_AGG_CELLS: 4097 rows x (1 + 16) percentile_ranks cells
    cells = {"h": {"type": "histogram", "field": "p4097", "interval": 0.5,
                   "aggs": {"r": {"type": "percentile_ranks", "field": "num", "values": list(range(16))}}}}
    fails(N.ERR_UNSUPPORTED, cells, "SLG_MAX_AGG_CELLS")
    # the one-shot without a value pointer refuses a spec with value nodes
    sp = A.agg_spec({"c": {"type": "cardinality", "field": "num"}}, W["fields"]).spec
    rc = ix._lib.slg_search_batch_aggs(ix._h, None, 0, None, None, None, C.addressof(sp), 11, 1, None, None, None,
                                       None, None, None, None)
    assert rc == N.ERR_INVALID and b"slg_search_batch_agg_values" in ix._lib.slg_last_error()
    # cursor and hybrid batches take no aggregations, value nodes included
    plan = A.agg_spec({"c": {"type": "cardinality", "field": "num"}}, W["fields"])
    for kw in (dict(cursors=[None] * 24), dict(hybrid=True)):
        with pytest.raises(N.SlgError) as ei:
            ix.prepare(W["offs"], W["terms"], W["w"], 11, aggs=plan, **kw)
        assert ei.value.code == N.ERR_UNSUPPORTED


def test_one_shot_with_value_tables(gpu, world):
    """slg_search_batch_agg_values = prepare + run + the three fetches"""
    from searchlite_amd import _native as N, aggs as A
    W = world
    ix = W["ix"]
    req = {"c": {"type": "cardinality", "field": "num"}, "t": {"type": "terms", "field": "kw8"}}
    plan = A.agg_spec(req, W["fields"])
    with ix.prepare(W["offs"], W["terms"], W["w"], 11, aggs=plan) as b:
        b.run()
        want = b.aggs()
        want_rows = b.fetch()
    nq, n_segs, k = 24, 3, 11
    qs = (N.Query * nq)()
    keep = []
    for q in range(nq):
        a, e = int(W["offs"][q]), int(W["offs"][q + 1])
        t = np.ascontiguousarray(W["terms"][a:e], dtype=np.uint32)
        ws = np.ascontiguousarray(W["w"][a:e], dtype=np.float32)
        keep += [t, ws]
        qs[q] = N.Query(e - a, t.ctypes.data, ws.ctypes.data)
    doc, seg = np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.uint32)
    score, count = np.zeros((nq, k), np.float32), np.zeros(nq, np.uint32)
    matched, counts, values = np.zeros(nq, np.uint64), np.zeros((nq, 8), np.uint64), np.zeros((nq, 1), np.uint64)
    p = lambda a: a.ctypes.data
    N.check(ix._lib.slg_search_batch_agg_values(ix._h, qs, nq, None, None, None, C.addressof(plan.spec), k, 1, p(doc),
                                                p(seg), p(score), p(count), p(matched), p(counts), None, p(values)))
    assert np.array_equal(values, want[0][:, 0, :]) and np.array_equal(counts, want[1][:, 0, :])
    assert np.array_equal(count, want_rows[3]) and matched.tolist() == [len(d) for d in W["docs"]]


def test_eight_nodes_run_twice(gpu, world):
    """SLG_MAX_AGGS nodes of every kind in one spec; two runs of one batch give identical tables, and the query
    that matches nothing all-zero ones"""
    from searchlite_amd import _native as N, aggs as A
    W = world
    req = {"a": {"type": "terms", "field": "kw8",
                 "aggs": {"a1": {"type": "cardinality", "field": "frac"},
                          "a2": {"type": "percentile_ranks", "field": "frac", "values": [0, 100.5]},
                          "a3": {"type": "stats", "field": "frac"}}},
           "b": {"type": "percentiles", "field": "frac"},
           "c": {"type": "percentiles", "field": "uniq", "percents": [10, 90]},
           "d": {"type": "cardinality", "field": "kwbig"},
           "e": {"type": "range", "field": "one", "ranges": [{"from": 3, "to": 3}]}}
    plan, tables, layout, _ = run_check(W, req, what="eight nodes")
    assert plan.spec.n_nodes == N.MAX_AGGS
    with W["ix"].prepare(W["offs"], W["terms"], W["w"], 11, aggs=plan) as b:
        b.run()
        first = b.aggs()
        b.run()
        second = b.aggs()
    for i, (t0, t1, t2) in enumerate(zip(tables, first, second)):
        assert t1.tobytes() == t2.tobytes() and t0.tobytes() == t1.tobytes(), f"node {i}: runs differ"
        assert t1[-1].tobytes() == bytes(t1[-1].nbytes), "the query that matches nothing has all-zero tables"


def test_ranks_across_index_updates(gpu, oracle):
    from searchlite_amd import _native as N, aggs as A
    rng = np.random.default_rng(12)
    segs = [random_segment(rng, 1200, 40, 20, k1=0.9, b=0.4), random_segment(rng, 700, 40, 20, k1=0.9, b=0.4)]
    offs, terms, w = random_queries(rng, 12, 3, 40, n_segs=2, weights=True)
    cols = make_columns(rng, segs)
    names = ["kw8", "num", "frac"]
    req = {"t": {"type": "terms", "field": "kw8", "aggs": {"c": {"type": "cardinality", "field": "num"}}},
           "p": {"type": "percentiles", "field": "frac"},
           "c": {"type": "cardinality", "field": "frac", "missing": 0.0001}}
    dead = rng.random(segs[0].n_docs) < 0.3
    bm = np.packbits(dead, bitorder="little")
    cur = [copy.copy(segs[0]), segs[1]]
    cur[0].deleted, cur[0].docs = bm, float(segs[0].n_docs - int(dead.sum()))
    docs = docs_of(oracle.search_batch(cur, offs, terms, w, 1900, strategy=oracle.BM25))
    with gpu.GpuIndex([copy.copy(s) for s in segs]) as ix:
        fields, ranks = register(ix, cols, names)
        W = dict(ix=ix, offs=offs, terms=terms, w=w, cols=cols, fields=fields,
                 docs=docs_of(oracle.search_batch(segs, offs, terms, w, 1900, strategy=oracle.BM25)))
        run_check(W, req, what="fresh")
        ix.update_deleted(0, bm, segs[0].n_docs - int(dead.sum()))
        W["docs"] = docs
        _, updated, _, _ = run_check(W, req, what="after update_deleted")
        assert [ix.rank_agg_field(fields[n]["id"]) for n in names] == [ranks[n] for n in names]
        with gpu.GpuIndex(cur) as fresh_ix:  # the same tables as a fresh staging of the new live set
            f2, r2 = register(fresh_ix, cols, names)
            assert r2 == ranks
            _, fresh, _, _ = run_check(dict(W, ix=fresh_ix, fields=f2), req, what="fresh staging")
        for a, b_ in zip(updated, fresh):
            assert a.tobytes() == b_.tobytes()
        # a segment added after the field: a batch that names it fails as it does for every aggregation
        extra = random_segment(rng, 500, 40, 20, k1=0.9, b=0.4)
        ix.add_segment(extra)
        terms3 = np.concatenate([terms, terms[:, :1]], axis=1)
        with pytest.raises(N.SlgError) as ei:
            ix.search_aggs(offs, terms3, w, 11, A.agg_spec(req, fields))
        assert ei.value.code == N.ERR_INVALID
        # registered and ranked again over the three segments; then one segment less: its ranks go, the
        # dictionary stays (a superset)
        cols3 = {n: cols[n] + make_columns(rng, [extra])[n] for n in names}
        f3, r3 = register(ix, cols3, names)
        W3 = dict(ix=ix, offs=offs, terms=terms3, w=w, cols=cols3, fields=f3,
                  docs=docs_of(oracle.search_batch(cur + [extra], offs, terms3, w, 2400, strategy=oracle.BM25)))
        run_check(W3, req, what="after add_segment, registered again")
        ix.remove_segment(1)
        cols2 = {n: [cols3[n][0], cols3[n][2]] for n in names}
        terms2 = np.ascontiguousarray(terms3[:, [0, 2]])
        W2 = dict(ix=ix, offs=offs, terms=terms2, w=w, cols=cols2, fields=f3,
                  docs=docs_of(oracle.search_batch([cur[0], extra], offs, terms2, w, 2400, strategy=oracle.BM25)))
        run_check(W2, req, what="after remove_segment")
        assert ix.rank_agg_field(f3["frac"]["id"]) == r3["frac"]
