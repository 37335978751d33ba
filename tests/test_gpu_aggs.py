"""Aggregations on the device (slg_index_add_agg_field_* + slg_batch_prepare_aggs).

The aggregated set of a query is what the oracle returns with k >= the number of docs (every accepted doc);
the expected tables are tests/agg_ref.py's collectors over that set, laid out densely.  Bar: counts, first_id
and stats equal (sums too: the columns hold exactly summable values, except in the general-doubles test), the
rows bit-identical to the same batch without aggregations, matched = the size of the set.
"""
import copy

import numpy as np
import pytest

from tests import agg_ref as R
from tests.util import load_golden, random_queries, random_segment

pytestmark = pytest.mark.gpu

NO_TERM = 0xFFFFFFFF
KEYS8 = [f"k{i}" for i in range(8)]
KEYS3000 = [f"t{i:04d}" for i in range(3000)]


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return sa


def tombstoned(seg, rng, frac):
    s = copy.copy(seg)
    dead = rng.random(seg.n_docs) < frac
    s.deleted = np.packbits(dead, bitorder="little")
    s.docs = float(seg.n_docs - int(dead.sum()))
    return s


def make_columns(rng, segs):
    """kw8 / kw3000: keyword fields of 8 / 3000 keys, 0-3 values per doc with repeats; num: i64 in [-50, 50],
    0-2 values; frac: f64 multiples of 2^-10 (sums are exact in any order), 0-2 values; one: i64 in [0, 9],
    0-1 value"""
    cols = {n: [] for n in ("kw8", "kw3000", "num", "frac", "one")}
    for s in segs:
        n = s.n_docs
        cols["kw8"].append([[KEYS8[j] for j in rng.integers(0, 8, int(rng.integers(0, 4)))] for _ in range(n)])
        cols["kw3000"].append([[KEYS3000[j] for j in rng.integers(0, 3000, int(rng.integers(0, 4)))]
                               for _ in range(n)])
        cols["num"].append([[int(x) for x in rng.integers(-50, 51, int(rng.integers(0, 3)))] for _ in range(n)])
        cols["frac"].append([[float(x) / 1024.0 for x in rng.integers(-(1 << 20), 1 << 20, int(rng.integers(0, 3)))]
                             for _ in range(n)])
        cols["one"].append([[int(x) for x in rng.integers(0, 10, int(rng.integers(0, 2)))] for _ in range(n)])
    return cols


KEYS_OF = {"kw8": KEYS8, "kw3000": KEYS3000}


def register(ix, cols, names=None):
    """-> the `fields` map of aggs.agg_spec"""
    fields = {}
    for name in names or cols:
        if name in KEYS_OF:
            ord_of = {k: i for i, k in enumerate(KEYS_OF[name])}
            per_seg = [[np.array([ord_of[v] for v in d], np.uint32) for d in seg] for seg in cols[name]]
            fields[name] = {"id": ix.add_agg_keyword_field(per_seg, len(ord_of)), "keys": KEYS_OF[name]}
        else:
            dt = np.float64 if name in ("frac", "normal") else np.int64
            fields[name] = {"id": ix.add_agg_field(cols[name], dt)}
    return fields


def docs_of(hits):
    doc, seg, _, count = hits
    return [[(int(seg[q, i]), int(doc[q, i])) for i in range(int(count[q]))] for q in range(len(count))]


@pytest.fixture(scope="module")
def world(gpu, oracle):
    rng = np.random.default_rng(2025)
    segs = [random_segment(rng, 3000, 60, 25, k1=0.9, b=0.4), random_segment(rng, 1500, 60, 25, k1=0.9, b=0.4),
            random_segment(rng, 800, 60, 25, k1=0.9, b=0.4)]
    segs[0] = tombstoned(segs[0], rng, 0.1)
    segs[2] = tombstoned(segs[2], rng, 0.2)
    offs, terms, w = random_queries(rng, 24, 3, 60, n_segs=3, weights=True)
    terms[-3:, :] = NO_TERM  # the last query matches nothing
    cols = make_columns(rng, segs)
    ix = gpu.GpuIndex(segs)
    fields = register(ix, cols)
    sort_id = ix.add_sort_field(cols["num"], np.int64)
    k_all = sum(s.n_docs for s in segs)
    all_hits = oracle.search_batch(segs, offs, terms, w, k_all, strategy=oracle.BM25)
    yield dict(ix=ix, segs=segs, offs=offs, terms=terms, w=w, cols=cols, fields=fields, k_all=k_all,
               docs=docs_of(all_hits), sort=[(sort_id, "asc"), ("_score", "desc")])
    ix.close()


_expected = {}


def expected(request, cols, docs, plan, key=None, keys_of=None):
    """agg_ref's tables of every query, computed once per (request, doc sets) and shared; keys_of: the keyword
    dictionaries of `cols` (KEYS_OF when not given)"""
    if key is not None and key in _expected:
        return _expected[key]
    keys_of = KEYS_OF if keys_of is None else keys_of
    layout = R.ref_layout(plan.nodes, cols, keys_of)
    per_q = [R.dense(plan.nodes, layout, R.run(request, cols, d), keys_of) for d in docs]
    out = layout, [np.stack([t[i] for t in per_q]) for i in range(len(plan.nodes))]
    if key is not None:
        _expected[key] = out
    return out


def check_tables(got_tables, got_layout, want_layout, want_tables, what="", sum_bound=None):
    for i, (g, w) in enumerate(zip(got_tables, want_tables)):
        gl, wl = got_layout[i], want_layout[i]
        assert (gl["parent_rows"], gl["rows"], gl["first_id"]) == (wl["parent_rows"], wl["rows"], wl["first_id"]), \
            f"{what} node {i}: layout {gl} != {wl}"
        assert g.shape == w.shape, f"{what} node {i}: shape {g.shape} != {w.shape}"
        if not gl["is_stats"]:
            assert np.array_equal(g, w), f"{what} node {i}: counts differ at {np.argwhere(g != w)[:5].tolist()}"
            continue
        for f in ("count", "min", "max"):
            assert np.array_equal(g[f], w[f]), f"{what} node {i}: stats {f} differ"
        if sum_bound is None:
            assert np.array_equal(g["sum"], w["sum"]), f"{what} node {i}: sums differ"
        else:
            err = np.abs(g["sum"] - w["sum"])
            print(f"{what} node {i}: max |sum - ref| {err.max():.3e}, smallest bound "
                  f"{sum_bound[sum_bound > 0].min() if (sum_bound > 0).any() else 0:.3e}")
            assert (err <= sum_bound.reshape(err.shape)).all(), f"{what} node {i}: sum beyond the bound"


def run_check(W, request, sort=None, k=11, docs=None, key=None, what="", **kw):
    """one aggregation batch against agg_ref and against the same batch without aggregations"""
    from searchlite_amd import aggs as A
    ix = W["ix"]
    plan = A.agg_spec(request, W["fields"])
    docs = W["docs"] if docs is None else docs
    want_layout, want_tables = expected(request, W["cols"], docs, plan, key, W.get("keys_of"))
    got = ix.search_aggs(W["offs"], W["terms"], W["w"], k, plan, sort=sort, **kw)
    doc, seg, score, count, matched, tables, layout = got
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
    check_tables(tables, layout, want_layout, want_tables, what)
    return plan, tables, layout


ROOTS = {
    "terms8": {"a": {"type": "terms", "field": "kw8"}},
    "terms8_missing_own": {"a": {"type": "terms", "field": "kw8", "missing": "none"}},
    "terms8_missing_k3": {"a": {"type": "terms", "field": "kw8", "missing": "k3"}},
    "terms3000": {"a": {"type": "terms", "field": "kw3000", "missing": "none"}},
    "histogram": {"a": {"type": "histogram", "field": "num", "interval": 7, "offset": 0.25}},
    "histogram_missing_bounds": {"a": {"type": "histogram", "field": "num", "interval": 10, "missing": 75,
                                       "hard_bounds": {"min": -20, "max": 80}}},
    "histogram_frac": {"a": {"type": "histogram", "field": "frac", "interval": 100.5, "offset": -3.0}},
    "range": {"a": {"type": "range", "field": "num", "missing": 0,
                    "ranges": [{"to": -10}, {"from": -10, "to": 10}, {"from": 10}, {"from": -50, "to": 50}]}},
    "stats": {"a": {"type": "stats", "field": "frac"}},
    "stats_missing": {"a": {"type": "stats", "field": "num", "missing": 3}},
}


@pytest.mark.parametrize("name", list(ROOTS))
def test_single_root_in_score_order_and_under_a_sort(gpu, world, name):
    for sort in (None, world["sort"]):
        run_check(world, ROOTS[name], sort=sort, key=name, what=f"{name} sort={sort is not None}")
    run_check(world, ROOTS[name], k=400, key=name, what=f"{name} k=400")


TWO_LEVEL = {
    "terms8_children": {"d": {"type": "terms", "field": "kw8", "missing": "none",
                              "aggs": {"s": {"type": "stats", "field": "frac"},
                                       "h": {"type": "histogram", "field": "num", "interval": 15},
                                       "t": {"type": "terms", "field": "kw8"}}}},
    "range_stats": {"r": {"type": "range", "field": "num", "ranges": [{"to": 0}, {"from": 0, "to": 25}, {"from": 20}],
                          "aggs": {"s": {"type": "stats", "field": "num", "missing": -1}}}},
    "eight_nodes": {"a": {"type": "terms", "field": "kw8",
                          "aggs": {"a1": {"type": "stats", "field": "num"},
                                   "a2": {"type": "range", "field": "frac", "ranges": [{"to": 0}, {"from": 0}]}}},
                    "b": {"type": "histogram", "field": "num", "interval": 25,
                          "aggs": {"b1": {"type": "terms", "field": "kw8", "missing": "k0"},
                                   "b2": {"type": "stats", "field": "frac", "missing": 0.5}}},
                    "c": {"type": "stats", "field": "one"},
                    "e": {"type": "range", "field": "one", "ranges": [{"from": 3, "to": 3}]}},
}


@pytest.mark.parametrize("name", list(TWO_LEVEL))
def test_two_levels(gpu, world, name):
    from searchlite_amd import _native as N
    plan, tables, layout = run_check(world, TWO_LEVEL[name], key=name, what=name)
    cells = sum(x["parent_rows"] * x["rows"] * (32 if x["is_stats"] else 4) for x in layout)
    assert cells <= N.AGG_LDS_BYTES, "these specs are meant for the LDS path"
    run_check(world, TWO_LEVEL[name], sort=world["sort"], key=name, what=name + " sorted")
    if name == "eight_nodes":
        assert plan.spec.n_nodes == N.MAX_AGGS


def test_large_tables_take_the_global_path(gpu, world):
    from searchlite_amd import _native as N
    req = {"h": {"type": "histogram", "field": "num", "interval": 10,
                 "aggs": {"t": {"type": "terms", "field": "kw3000"}}}}
    plan, tables, layout = run_check(world, req, key="hist_terms3000", what="histogram -> terms(3000)")
    cells = sum(x["parent_rows"] * x["rows"] for x in layout if not x["is_stats"])
    assert layout[1]["parent_rows"] == 11 and layout[1]["rows"] == 3000
    assert 4 * cells > N.AGG_LDS_BYTES and cells <= N.MAX_AGG_CELLS
    req = {"t": {"type": "terms", "field": "kw3000", "aggs": {"s": {"type": "stats", "field": "frac"}}}}
    plan, tables, layout = run_check(world, req, sort=world["sort"], key="terms3000_stats", what="terms(3000) -> stats")
    assert 32 * layout[1]["parent_rows"] > N.AGG_LDS_BYTES


def test_child_counts_sum_to_the_parent(gpu, world):
    """a single-valued child with `missing` puts every doc of a parent bucket into exactly one child bucket"""
    req = {"d": {"type": "terms", "field": "kw8", "missing": "none",
                 "aggs": {"h": {"type": "histogram", "field": "one", "interval": 2, "missing": 20}}}}
    plan, tables, layout = run_check(world, req, key="consistency", what="consistency")
    parent, child = tables[0], tables[1]  # [nq, 1, 9], [nq, 9, rows]
    assert np.array_equal(child.sum(axis=2), parent[:, 0, :])
    assert parent.sum() > 0


def test_filter_min_match_plans_and_many_terms(gpu, world, oracle):
    W = world
    rng = np.random.default_rng(7)
    req = TWO_LEVEL["terms8_children"]
    masks = [rng.random(s.n_docs) < 0.5 for s in W["segs"]]
    fid = W["ix"].add_filter(masks)
    nq = len(W["offs"]) - 1
    qf = np.where(np.arange(nq) % 2 == 0, fid, -1).astype(np.int32)
    want = oracle.search_batch_filtered(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], qf, {fid: masks},
                                        strategy=oracle.BM25)
    run_check(W, req, docs=docs_of(want), what="filter", q_filter=qf)
    run_check(W, req, docs=docs_of(want), sort=W["sort"], what="filter sorted", q_filter=qf)
    mm = np.where(np.arange(nq) % 3 == 0, 2, 0).astype(np.uint32)
    want = oracle.search_batch_min_match(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], mm,
                                         strategy=oracle.BM25, q_filter=qf, filters={fid: masks})
    run_check(W, req, docs=docs_of(want), what="min_match", q_filter=qf, q_min_match=mm)
    W["ix"].remove_filter(fid)
    two = dict(q_nleaves=np.full(nq, 3, np.uint32), q_plan=np.zeros(nq, np.int32),
               q_leaf_offsets=(np.arange(nq + 1) * 3).astype(np.uint32),
               leaf_group=np.tile(np.array([0, 0, 1], np.uint32), nq),
               q_group_offsets=(np.arange(nq + 1) * 2).astype(np.uint32),
               group_plan=np.tile(np.array([1, 0], np.int32), nq),
               group_tie=np.tile(np.array([0.3, 0.0], np.float32), nq))
    run_check(W, req, what="two-level plan", key="terms8_children", **two)  # (the plan changes scores, not the set)


def test_twelve_term_queries_on_the_many_term_kernel(gpu, oracle):
    rng = np.random.default_rng(312)
    segs = [random_segment(rng, 2000, 80, 30, k1=0.9, b=0.4), random_segment(rng, 900, 80, 30, k1=0.9, b=0.4)]
    offs, terms, w = random_queries(rng, 8, 12, 80, n_segs=2, weights=True)
    cols = make_columns(rng, segs)
    want = oracle.search_batch(segs, offs, terms, w, 2900, strategy=oracle.BM25)
    with gpu.GpuIndex(segs) as ix:
        W = dict(ix=ix, segs=segs, offs=offs, terms=terms, w=w, cols=cols, docs=docs_of(want),
                 fields=register(ix, cols, ["kw8", "num", "frac"]))
        run_check(W, TWO_LEVEL["terms8_children"], what="12 terms")


def test_empty_query_and_repeat_runs(gpu, world):
    from searchlite_amd import aggs as A
    W = world
    assert W["docs"][-1] == []
    for req in (TWO_LEVEL["eight_nodes"], {"t": {"type": "terms", "field": "kw3000",
                                                 "aggs": {"s": {"type": "stats", "field": "frac"}}}}):
        plan = A.agg_spec(req, W["fields"])
        with W["ix"].prepare(W["offs"], W["terms"], W["w"], 11, aggs=plan) as b:
            b.run()
            first = b.aggs()
            b.run()
            second = b.aggs()
        for t1, t2 in zip(first, second):
            assert t1[-1].tobytes() == bytes(t1[-1].nbytes), "the query that matches nothing has all-zero tables"
            assert t1.tobytes() == t2.tobytes(), "a batch run twice gives identical tables"


def test_general_doubles_sum_bound(gpu, oracle):
    """standard-normal values: counts, min and max exact; |sum - ref| <= 2 (n - 1) 2^-53 sum|x|, the worst-case
    distance of two summation orders of the same n doubles (each within (n - 1) u sum|x| of the exact sum)."""
    from searchlite_amd import aggs as A
    rng = np.random.default_rng(5)
    segs = [random_segment(rng, 2500, 40, 20, k1=0.9, b=0.4), random_segment(rng, 700, 40, 20, k1=0.9, b=0.4)]
    offs, terms, w = random_queries(rng, 12, 3, 40, n_segs=2, weights=True)
    cols = make_columns(rng, segs)
    cols["normal"] = [[[float(x) for x in rng.standard_normal(int(rng.integers(0, 3)))] for _ in range(s.n_docs)]
                      for s in segs]
    docs = docs_of(oracle.search_batch(segs, offs, terms, w, 3200, strategy=oracle.BM25))
    req = {"s": {"type": "stats", "field": "normal"},
           "t": {"type": "terms", "field": "kw8", "aggs": {"s": {"type": "stats", "field": "normal"}}}}
    with gpu.GpuIndex(segs) as ix:
        fields = register(ix, cols, ["kw8", "normal"])
        plan = A.agg_spec(req, fields)
        want_layout, want_tables = expected(req, cols, docs, plan)
        *_, tables, layout = ix.search_aggs(offs, terms, w, 11, plan)
        for i, nd in enumerate(plan.nodes):
            if nd["type"] != "stats":
                check_tables([tables[i]], [layout[i]], [want_layout[i]], [want_tables[i]], nd["name"])
                continue
            # n and sum|x| of every cell: the same collectors over |x|
            abs_cols = dict(cols, normal=[[[abs(v) for v in d] for d in seg] for seg in cols["normal"]])
            _, abs_tables = expected(req, abs_cols, docs, plan)
            n = want_tables[i]["count"].astype(np.float64)
            bound = 2.0 * np.maximum(n - 1.0, 0.0) * 2.0 ** -53 * abs_tables[i]["sum"]
            check_tables([tables[i]], [layout[i]], [want_layout[i]], [want_tables[i]], f"normal {nd['name']}",
                         sum_bound=bound)


def test_lifecycle_and_errors(gpu, oracle):
    from searchlite_amd import _native as N, aggs as A
    rng = np.random.default_rng(11)
    segs = [random_segment(rng, 1200, 40, 20, k1=0.9, b=0.4), random_segment(rng, 700, 40, 20, k1=0.9, b=0.4)]
    offs, terms, w = random_queries(rng, 12, 3, 40, n_segs=2, weights=True)
    cols = make_columns(rng, segs)
    req = TWO_LEVEL["terms8_children"]
    with gpu.GpuIndex([copy.copy(s) for s in segs]) as ix:
        fields = register(ix, cols, ["kw8", "num", "frac"])
        W = dict(ix=ix, segs=segs, offs=offs, terms=terms, w=w, cols=cols, fields=fields,
                 docs=docs_of(oracle.search_batch(segs, offs, terms, w, 1900, strategy=oracle.BM25)))
        run_check(W, req, what="fresh")
        # update_deleted keeps the columns: the tables of the new live set
        dead = rng.random(segs[0].n_docs) < 0.3
        bm = np.packbits(dead, bitorder="little")
        ix.update_deleted(0, bm, segs[0].n_docs - int(dead.sum()))
        cur = [copy.copy(segs[0]), segs[1]]
        cur[0].deleted, cur[0].docs = bm, float(segs[0].n_docs - int(dead.sum()))
        W["docs"] = docs_of(oracle.search_batch(cur, offs, terms, w, 1900, strategy=oracle.BM25))
        run_check(W, req, what="after update_deleted")

        def fails(code, request=req, flds=None, t=terms, **kw):
            with pytest.raises(N.SlgError) as ei:
                ix.search_aggs(offs, t, w, 11, A.agg_spec(request, flds or fields), **kw)
            assert ei.value.code == code, ei.value

        # a column with a NaN registers, a batch that names it is unsupported
        bad = [[list(d) for d in seg] for seg in cols["frac"]]
        bad[1][5] = [float("nan")]
        nan_id = ix.add_agg_field(bad, np.float64)
        fails(N.ERR_UNSUPPORTED, {"s": {"type": "stats", "field": "x"}}, {"x": {"id": nan_id}})
        # a field of the wrong kind for its node; missing_ord beyond the dictionary
        fails(N.ERR_INVALID, {"s": {"type": "stats", "field": "kw8"}})
        fails(N.ERR_INVALID, {"t": {"type": "terms", "field": "num"}})
        sp = A.agg_spec({"t": {"type": "terms", "field": "kw8", "missing": "none"}}, fields)
        sp.spec.nodes[0].missing_ord = 9
        with pytest.raises(N.SlgError) as ei:
            ix.search_aggs(offs, terms, w, 11, sp)
        assert ei.value.code == N.ERR_INVALID
        # more than SLG_MAX_AGG_CELLS cells: 3000 x 3000 count cells; 65 536 histogram buckets
        big = register(ix, {"kw3000": [[[] for _ in range(s.n_docs)] for s in segs]}, ["kw3000"])
        fails(N.ERR_UNSUPPORTED, {"t": {"type": "terms", "field": "kw3000",
                                        "aggs": {"u": {"type": "terms", "field": "kw3000"}}}}, big)
        fails(N.ERR_UNSUPPORTED, {"h": {"type": "histogram", "field": "num", "interval": 0.001}})
        # aggregations asked of a cursor batch or a hybrid batch
        plan = A.agg_spec(req, fields)
        for kw in (dict(cursors=[None] * 12), dict(hybrid=True)):
            with pytest.raises(N.SlgError) as ei:
                ix.prepare(offs, terms, w, 11, aggs=plan, **kw)
            assert ei.value.code == N.ERR_UNSUPPORTED
        # a segment added after the fields: no column for it
        extra = random_segment(rng, 500, 40, 20, k1=0.9, b=0.4)
        ix.add_segment(extra)
        terms3 = np.concatenate([terms, terms[:, :1]], axis=1)
        fails(N.ERR_INVALID, t=terms3)
        cols3 = {n: cols[n] + make_columns(rng, [extra])[n] for n in ("kw8", "num", "frac")}
        fields3 = register(ix, cols3)
        assert min(f["id"] for f in fields3.values()) > max(f["id"] for f in fields.values())
        W3 = dict(ix=ix, offs=offs, terms=terms3, w=w, cols=cols3, fields=fields3,
                  docs=docs_of(oracle.search_batch(cur + [extra], offs, terms3, w, 2400, strategy=oracle.BM25)))
        run_check(W3, req, what="after add_segment")
        # a removed id is unknown, and ids are never handed out again
        gone = fields3["num"]["id"]
        ix.remove_agg_field(gone)
        again = ix.add_agg_field(cols3["num"], np.int64)
        assert again > max(f["id"] for f in fields3.values())
        fails(N.ERR_INVALID, flds=fields3, t=terms3)
        fails(N.ERR_INVALID, {"s": {"type": "stats", "field": "x"}}, {"x": {"id": 12345}}, t=terms3)
        with pytest.raises(N.SlgError) as ei:
            ix.remove_agg_field(gone)
        assert ei.value.code == N.ERR_INVALID
        run_check(dict(W3, fields=dict(fields3, num={"id": again})), req, what="registered again")
        with ix.prepare(offs, terms3, w, 11) as b:  # a batch without aggregations has no tables
            b.run()
            assert ix._lib.slg_batch_fetch_aggs(b._h, None, None) == N.ERR_INVALID


def test_recipes_example_request(gpu, oracle):
    """examples/recipes/queries/agg-macros-by-diet.json's aggregations over the recipes corpus: terms on
    dietary_tags (size 8) with protein stats and a total_time_minutes histogram of interval 15, and the range
    aggregation; through search_aggs + aggs.shape against agg_ref's response."""
    import os
    from searchlite_amd import aggs as A
    segs, z = load_golden("recipes.npz")
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    ag, so = np.load(os.path.join(gold, "recipes_aggs.npz")), np.load(os.path.join(gold, "recipes_sort.npz"))
    keys = [str(k) for k in ag["diet_keys"]]
    n = segs[0].n_docs
    csr = lambda o, v, f: [[f(x) for x in v[o[d]:o[d + 1]]] for d in range(n)]
    cols = {"dietary_tags": [csr(ag["diet_offsets"], ag["diet_ords"], lambda x: keys[int(x)])],
            "nutrition.per_serving.protein_g": [csr(ag["protein_offsets"], ag["protein"], float)],
            "total_time_minutes": [csr(so["total_time_minutes_offsets"], so["total_time_minutes"], int)]}
    req = {"by_diet": {"type": "terms", "field": "dietary_tags", "size": 8,
                       "aggs": {"protein_stats": {"type": "stats", "field": "nutrition.per_serving.protein_g"},
                                "time_buckets": {"type": "histogram", "field": "total_time_minutes", "interval": 15}}},
           "fast_meals": {"type": "range", "field": "total_time_minutes",
                          "ranges": [{"to": 20}, {"from": 20, "to": 40}, {"from": 40}]}}
    qo, qt, qw = z["q_offsets"], z["q_terms"], z["q_weights"]
    docs = docs_of(oracle.search_batch(segs, qo, qt, qw, n, strategy=oracle.BM25))
    with gpu.GpuIndex(segs) as ix:
        fields = {"dietary_tags": {"id": ix.add_agg_keyword_field([(ag["diet_offsets"], ag["diet_ords"])], len(keys)),
                                   "keys": keys},
                  "nutrition.per_serving.protein_g": {"id": ix.add_agg_field([(ag["protein_offsets"], ag["protein"])],
                                                                             np.float64)},
                  "total_time_minutes": {"id": ix.add_agg_field([(so["total_time_minutes_offsets"],
                                                                  so["total_time_minutes"])], np.int64)}}
        plan = A.agg_spec(req, fields)
        *_, matched, tables, layout = ix.search_aggs(qo, qt, qw, 2, plan)
        assert any(len(d) > 0 for d in docs)
        for q, d in enumerate(docs):
            assert int(matched[q]) == len(d)
            assert A.shape(plan, layout, tables, q) == R.respond(req, R.run(req, cols, d)), f"query {q}"
