"""Scan batches on the device (slg_batch_prepare_scan, slg_search_batch_scan: match_all, constant_score and
rank_feature at the root) through the C ABI against tests/scan_ref.py.  Tolerance 0: docs, segments, scores (bit
patterns), counts, scored_docs, matched counts and every aggregation table are identical to the reference; rows past
the count are zero.  The stats sums are compared for equality too: the columns they run over hold multiples of 2^-10,
whose sums are exact in every order, so the bound of the aggregation tests is met with 0.

How tolerance 0 is reached: the only operations that are not correctly rounded are the f64 ln and log1p, whose result
is then rounded to f32.  The worlds keep only column values whose result is `safe` (scan_ref.safe: further than 2^-40
relative from an f32 rounding boundary); unsafe draws are replaced on the CPU (at most 1 % of them), and every check
asserts with the reference alone, before the device is touched, that none is left."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import scan_ref as R
from tests.test_gpu_bool import same
from tests.test_gpu_sort import check as check_sorted

pytestmark = pytest.mark.gpu
F32 = np.float32

MA = {"match_all": {}}
CS = lambda **kw: {"constant_score": kw}
RF = lambda field, **kw: {"rank_feature": dict(field=field, **kw)}
# every transcendental query the tests put on the random column `pop`: the column is made safe for exactly these
LOGS = [dict(modifier=m, boost=b) for m in ("log", "log1p") for b in (1.0, -0.5, 3.0)]
EDGE_VALUES = [0.0, -0.0, -1.0, float(np.nextafter(-1.0, -2.0)), float(np.nextafter(-1.0, 0.0)), -5.0,
               float(np.nextafter(0.0, 1.0)), float(np.nextafter(0.0, -1.0)), 1e308, -1e308, 1e39, 3e38, 4.0, 0.25, 1e-3]


def bare_segment(n, dead=None):
    """a segment of n docs with one posting (a scan reads no posting list); dead: bool array or None"""
    from searchlite_amd.segment import Segment
    return Segment(n_docs=n, term_offsets=np.array([0, 1], np.uint64), doc_ids=np.array([0], np.uint32),
                   tfs=np.array([1], np.uint32), field_doc_len=[np.ones(n, F32)], field_avgdl=np.array([1.0], F32),
                   docs=float(n - (0 if dead is None else int(dead.sum()))),
                   deleted=None if dead is None else np.packbits(dead, bitorder="little"))


class World:
    """bare segments, an index over them, registered columns and filters (by name), and scan_ref's view of them"""

    def __init__(self, sa, sizes, dead, **tuning):
        self.sizes = list(sizes)
        self.segs = [bare_segment(n, d) for n, d in zip(sizes, dead)]
        self.ix = sa.GpuIndex(self.segs, **tuning)
        self.ref = dict(n_docs=self.sizes, deleted=list(dead), filters={}, fields={})
        self.F, self.flt = {}, {}
        self.D = self.slice_docs()

    def slice_docs(self):
        with self.ix.prepare_scan([MA], 0) as b:
            return b.info()["scan_slice_docs"]

    def add_field(self, name, per_seg, dtype):
        self.F[name] = fid = self.ix.add_agg_field(per_seg, dtype)
        self.ref["fields"][fid] = per_seg
        return fid

    def add_filter(self, name, masks):
        self.flt[name] = fid = self.ix.add_filter(masks)
        self.ref["filters"][fid] = masks
        return fid

    def named(self, query):
        """the query with its field and filter names replaced by the ids of this world"""
        (name, body), = query.items()
        body = dict(body)
        if isinstance(body.get("field"), str):
            body["field"] = self.F[body["field"]]
        if isinstance(body.get("filter"), str):
            body["filter"] = self.flt[body["filter"]]
        return {name: body}

    def want(self, queries, k, q_filter=None):
        queries = [self.named(q) for q in queries]
        assert not R.unsafe_docs(queries, self.ref), "a column value is too close to an f32 rounding boundary"
        return (queries,) + R.search(queries, self.ref, k, q_filter)

    def check(self, queries, k, what, q_filter=None):
        """a scan batch in score order, with stats -> (rows, matched, per query hits)"""
        qf = None if q_filter is None else np.array([self.flt.get(f, -1) if isinstance(f, str) else f for f in q_filter], np.int32)
        queries, want, matched, per_q = self.want(queries, k, qf)
        got = self.ix.search_scan(queries, k, q_filter=qf, want_stats=True)
        same(got[:4], want, what)
        nq = len(queries)
        assert got[5].tolist() == matched.tolist(), f"{what}: matched {got[5].tolist()} != {matched.tolist()}"
        assert [int(got[4][q].scored_docs) for q in range(nq)] == matched.tolist(), f"{what}: scored_docs"
        assert [int(got[4][q].candidates_examined) for q in range(nq)] == matched.tolist()
        return want, matched, per_q


def safe_values(rng, draw, sizes, specs):
    """per segment one value list per doc from draw(); the draws some rank_feature of `specs` (over field 0) turns
    into an unsafe f64 are drawn again -> per_seg, with at most 1 % of the draws replaced"""
    per_seg = [[draw() for _ in range(n)] for n in sizes]
    w = dict(n_docs=list(sizes), deleted=[None] * len(sizes), filters={}, fields={0: per_seg})
    replaced = 0
    for _ in range(20):
        w.pop("_first", None)
        bad = R.unsafe_docs([RF(0, **s) for s in specs], w)
        if not bad:
            break
        for _, s, d in bad:
            per_seg[s][d] = draw()
            replaced += 1
    assert not bad and replaced <= sum(sizes) // 100, (replaced, sum(sizes))
    return per_seg


def planned_slice_docs():
    """D, the docs per slice the planner cuts at, from the host planner's library: no device"""
    from searchlite_amd import build
    L = C.CDLL(build.build_plan_lib())
    L.slgp_scan_slice_docs.restype = C.c_uint32
    return int(L.slgp_scan_slice_docs())


def run_of(n, lo, hi):
    m = np.zeros(n, bool)
    m[lo:hi] = True
    return m


@pytest.fixture(scope="module")
def A():
    """fifteen segments around every size at which the kernel takes another path (the 32-doc word, the 64-doc round,
    the 2048-doc step, the slice of D docs), one of three full slices (3D docs) and the last of 2D + 5.  Tombstones
    in the odd segments and the last, `deleted` null in the other even ones.  Columns: `pop` f64 with 0-2 values per doc (offsets), `one` f64 and `age` i64 with one
    value per doc (stored without offsets), `edge` f64 over the branch edges of the modifiers.  Filters: see below"""
    import searchlite_amd as sa
    rng = np.random.default_rng(61)
    D = planned_slice_docs()
    sizes = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, D - 1, D, D + 1, 3 * D, 2 * D + 5]
    last = len(sizes) - 1
    dead = [(rng.random(n) < 0.2) if (i % 2 or i == last) else None for i, n in enumerate(sizes)]
    dead[-1][20:45] = dead[-1][D - 10:D + 10] = False  # (the runs of filter `runs` stay whole in the last segment)
    # the columns first: what the reference asserts about them is asserted before a device is touched
    columns = {"pop": (safe_values(rng, lambda: [float(rng.uniform(0.1, 1000.0)) for _ in range(int(rng.integers(0, 3)))],
                                   sizes, LOGS), np.float64),
               "one": ([[[float(rng.integers(0, 64)) / 8.0] for _ in range(n)] for n in sizes], np.float64),
               "age": ([[[int(rng.integers(-50, 5001))] for _ in range(n)] for n in sizes], np.int64),
               "edge": ([[[EDGE_VALUES[int(rng.integers(0, len(EDGE_VALUES)))]] if rng.random() < 0.9 else []
                          for _ in range(n)] for n in sizes], np.float64)}
    by_name = dict(n_docs=sizes, deleted=dead, filters={}, fields={name: v for name, (v, _) in columns.items()})
    assert not R.unsafe_docs(KINDS, by_name), "a column value is too close to an f32 rounding boundary"
    Wd = World(sa, sizes, dead)
    assert Wd.D == D
    Wd.trunc = sizes.index(3 * D)  # the segment of three full slices (the truncation edges)
    for name, (per_seg, dtype) in columns.items():
        Wd.add_field(name, per_seg, dtype)
    Wd.add_filter("all", [np.ones(n, bool) for n in sizes])
    Wd.add_filter("none", [np.zeros(n, bool) for n in sizes])
    Wd.add_filter("first", [run_of(n, 0, 1) for n in sizes])
    Wd.add_filter("last", [run_of(n, n - 1, n) for n in sizes])
    Wd.add_filter("even", [np.arange(n) % 2 == 0 for n in sizes])
    Wd.add_filter("odd", [np.arange(n) % 2 == 1 for n in sizes])
    # a run across a word boundary (docs 20 .. 44) and, in the last segment, across the slice boundary (D - 10 .. D + 9)
    Wd.add_filter("runs", [run_of(n, 20, 45) | (run_of(n, D - 10, D + 10) if i == last else False) for i, n in enumerate(sizes)])
    Wd.add_filter("half", [rng.random(n) < 0.5 for n in sizes])
    Wd.add_filter("tenth", [rng.random(n) < 0.1 for n in sizes])
    Wd.rng = rng
    yield Wd
    Wd.ix.close()


@pytest.fixture(scope="module")
def B():
    """three segments in one index (3000, 2049 and 700 docs): tombstones in the first, `deleted` null in the others;
    filter `no1` passes no doc of segment 1.  The aggregation columns of tests/test_gpu_aggs.py (keyword fields of 8
    and 3000 keys, `num`, `frac` with exact sums, `one`), `num` ranked for cardinality; sort fields `low` (i64, 8
    values: ties across every k) and `f` (f64, some docs without a value); `pop` as in world A"""
    import searchlite_amd as sa
    from tests.test_gpu_aggs import make_columns, register
    rng = np.random.default_rng(67)
    sizes = [3000, 2049, 700]
    # (drawn, and its replaced share asserted with the reference alone, before a device is touched)
    pop = safe_values(rng, lambda: [float(rng.uniform(0.1, 1000.0)) for _ in range(int(rng.integers(0, 3)))], sizes, LOGS)
    Wd = World(sa, sizes, [rng.random(3000) < 0.15, None, None])
    Wd.cols = make_columns(rng, Wd.segs)
    Wd.fields = register(Wd.ix, Wd.cols)
    Wd.ix.rank_agg_field(Wd.fields["num"]["id"])
    Wd.add_field("pop", pop, np.float64)
    low = [[[int(rng.integers(0, 8))] for _ in range(n)] for n in sizes]
    f = [[[float(rng.integers(-40, 40)) / 4.0] if rng.random() < 0.8 else [] for _ in range(n)] for n in sizes]
    Wd.ref["sort_fields"] = {"low": low, "f": f}
    Wd.sort_id = {"low": Wd.ix.add_sort_field(low, np.int64), "f": Wd.ix.add_sort_field(f, np.float64)}
    Wd.add_filter("no1", [rng.random(3000) < 0.5, np.zeros(2049, bool), rng.random(700) < 0.5])
    Wd.add_filter("third", [rng.random(n) < 0.33 for n in sizes])
    yield Wd
    Wd.ix.close()


KINDS = [MA, CS(boost=2.5), CS(filter="half", boost=-1.5, node_boost=2.0), RF("pop", modifier="log1p"),
         RF("pop", modifier="log", boost=-0.5, missing=2.0), RF("one", modifier="sqrt", boost=2.0), RF("age"),
         RF("age", modifier="reciprocal", boost=3.0), RF("edge", modifier="log1p", boost=1.0), RF("edge", modifier="log"),
         RF("edge", modifier="sqrt"), RF("edge", modifier="reciprocal"), RF("edge", boost=2.0, missing=-3.5)]


# ---- sizes, kinds, kernels -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [11, 1025])
def test_every_segment_size_and_the_three_kinds_in_one_batch(A, k):
    """columns with offsets (`pop`), without (`one`, `edge`) and from i64 (`age`); tombstones and null `deleted`"""
    want, matched, _ = A.check(KINDS, k, f"kinds k={k}")
    live = sum(n if d is None else int((~d).sum()) for n, d in zip(A.sizes, A.ref["deleted"]))
    assert matched[0] == matched[1] == live and 0 < matched[2] < live
    assert matched[11] < live, "reciprocal of the smallest subnormal is inf: those docs are dropped"
    assert (want[2][0, :want[3][0]] == F32(1.0)).all() and (want[2][1, :want[3][1]] == F32(2.5)).all()


def test_each_kernel_instantiation_on_purpose(A):
    lean = [MA, CS(boost=0.5), RF("one"), RF("one", modifier="sqrt"), RF("age", modifier="reciprocal")]
    with A.ix.prepare_scan([A.named(q) for q in lean], 11) as b:
        info = b.info()
        assert info["scan_kernel"] == "lean" and info["n_postings"] == 0
        per_query = sum((n + A.D - 1) // A.D for n in A.sizes)
        assert info["n_slices"] == per_query * len(lean) and per_query == len(A.sizes) + 1 + 2 + 2
    A.check(lean, 11, "lean")
    for m in ("log", "log1p"):
        with A.ix.prepare_scan([A.named(q) for q in lean + [RF("pop", modifier=m)]], 11) as b:
            assert b.info()["scan_kernel"] == "full"
        A.check(lean + [RF("pop", modifier=m)], 11, f"full {m}")


# ---- pass patterns -----------------------------------------------------------------------------------------
def test_pass_patterns(A):
    """all, none, only the first doc, only the last doc, every other doc, runs across a word and a slice boundary —
    as the node's filter, as the root filter and as both; the patterns are asserted on the CPU first"""
    n_segs, last = len(A.sizes), len(A.sizes) - 1
    live = lambda s: np.ones(A.sizes[s], bool) if A.ref["deleted"][s] is None else ~A.ref["deleted"][s]
    count = lambda name: sum(int((A.ref["filters"][A.flt[name]][s] & live(s)).sum()) for s in range(n_segs))
    names = ["all", "none", "first", "last", "even", "runs"]
    queries = [CS(filter=nm, boost=1.0 + i) for i, nm in enumerate(names)]
    _, matched, per_q = A.want(queries, 0)[1:]
    assert matched.tolist() == [count(nm) for nm in names]
    assert matched[1] == 0 and matched[2] <= n_segs and matched[3] <= n_segs and matched[0] == sum(int(live(s).sum()) for s in range(n_segs))
    assert all(d == 0 for d in per_q[2][1].tolist()) and per_q[3][1].tolist() == [A.sizes[s] - 1 for s in per_q[3][0].tolist()]
    runs_last = per_q[5][1][per_q[5][0] == last]
    assert {A.D - 1, A.D}.issubset(runs_last.tolist()) and {31, 32}.issubset(runs_last.tolist())  # both boundaries are crossed
    for k in (11, 1025):
        A.check(queries, k, f"node filters k={k}")
        A.check([MA] * len(names), k, f"root filters k={k}", q_filter=names)
        A.check([RF("one", filter=nm) for nm in names], k, f"rank_feature node filters k={k}")


def test_node_and_root_filters_overlapping_disjoint_and_equal(A):
    pairs = [("half", "tenth"), ("even", "odd"), ("half", "half"), ("even", "runs"), ("all", "none"), ("first", "last")]
    queries = [CS(filter=a, boost=2.0) for a, _ in pairs]
    _, matched, _ = A.want(queries, 0, np.array([A.flt[b] for _, b in pairs], np.int32))[1:]
    only_node = A.want(queries, 0)[2]
    assert matched[1] == 0 and matched[4] == 0 and matched[2] == only_node[2] and 0 < matched[0] < only_node[0]
    assert matched[5] == 1  # (the one-doc segment: its first doc is its last)
    for k in (0, 11, 1025):
        A.check(queries, k, f"node and root k={k}", q_filter=[b for _, b in pairs])
        A.check([RF("pop", modifier="log1p", filter=a) for a, _ in pairs], k, f"rank_feature node and root k={k}",
                q_filter=[b for _, b in pairs])


# ---- truncation --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 11, 257, 1025])
def test_truncated_regions_keep_exact_counts(A, k):
    """slices with exactly k - 1, k and k + 1 passing docs — the three full slices of the 3D-doc segment, which has
    tombstones — spread over their slice, packed at its end (the run crosses the region's capacity inside one
    64-doc round) and packed at its start (every later step only counts); the regions hold min(slice docs, k)
    candidates, the counts stay exact.  The three counts of every pattern are asserted on the CPU first"""
    t, D, n = A.trunc, A.D, A.sizes[A.trunc]
    assert n == 3 * D and A.ref["deleted"][t] is not None
    live = ~A.ref["deleted"][t]
    per_slice = [max(k - 1, 0), k, k + 1]
    patterns = {"spread": np.zeros(n, bool), "packed": np.zeros(n, bool), "front": np.zeros(n, bool)}
    for i, want_n in enumerate(per_slice):
        docs = np.nonzero(live[i * D:(i + 1) * D])[0] + i * D
        assert len(docs) > want_n
        patterns["spread"][docs[np.unique(np.linspace(0, len(docs) - 1, want_n).astype(int))] if want_n else []] = True
        patterns["packed"][docs[len(docs) - want_n:] if want_n else []] = True
        patterns["front"][docs[:want_n] if want_n else []] = True
    masks = lambda m: [m if s == t else np.zeros(sz, bool) for s, sz in enumerate(A.sizes)]
    for name, m in patterns.items():
        assert [int((m & live)[i * D:(i + 1) * D].sum()) for i in range(3)] == per_slice, f"the pattern itself: {name}"
        A.add_filter(f"{name}{k}", masks(m))
    queries = [CS(filter=f"spread{k}", boost=3.0), CS(filter=f"packed{k}"), CS(filter=f"front{k}", boost=0.5),
               {"match_all": {"filter": f"spread{k}"}}, MA]
    try:
        _, matched, _ = A.check(queries, k, f"truncated k={k}")
        assert matched[:4].tolist() == [sum(per_slice)] * 4
        A.check([MA, CS(boost=2.0), MA], k, f"truncated root k={k}", q_filter=[f"packed{k}", f"spread{k}", f"front{k}"])
    finally:
        for name in patterns:
            A.ix.remove_filter(A.flt.pop(f"{name}{k}"))


# ---- sorts -------------------------------------------------------------------------------------------------
def sorted_rows(Wd, queries, sort, q_filter=None):
    """every hit of every query in the sort's order, with the score the device reports (scan_ref.search_sorted)"""
    return [rows for rows, _ in R.search_sorted(queries, Wd.ref, sum(Wd.sizes), sort, q_filter, device=True)]


@pytest.mark.parametrize("sort", [[("low", "asc")], [("low", "desc")], [("f", "asc"), ("_score", "desc")],
                                  [("_score", "desc"), ("low", "asc")], [("_score", "asc")]],
                         ids=lambda s: "+".join(f"{p}:{o}" for p, o in s))
def test_field_sorts_and_the_documented_zero_score(B, sort):
    """one field sort in each order and `_score` as a part.  Without a `_score` part every row's score is 0.0 (the
    sorted select's rule; the reference would report a constant_score or rank_feature hit's computed score:
    the one known deviation) — check_sorted asserts the zeros"""
    queries = [B.named(q) for q in (MA, CS(filter="third", boost=2.0), RF("pop", modifier="log1p"),
                                    RF("pop", modifier="reciprocal", filter="no1"), CS(filter="no1"))]
    qf = np.array([-1, -1, B.flt["third"], -1, B.flt["third"]], np.int32)
    matched = B.want(queries, 0, qf)[2]
    rows = sorted_rows(B, queries, sort, qf)
    if not any(p == "_score" for p, _ in sort):
        assert all(float(h[2]) == 0.0 for hits in rows for h in hits) and any(len(hits) for hits in rows)
    dev_sort = [(p if p == "_score" else B.sort_id[p], o) for p, o in sort]
    for k in (0, 11, 257):
        got = B.ix.search_scan(queries, k, sort=dev_sort, q_filter=qf)
        check_sorted(got, rows, k, sort, f"sorted k={k}")
        assert got[4].tolist() == matched.tolist()


# ---- aggregations ------------------------------------------------------------------------------------------
REQUESTS = {
    "terms_stats_lds": {"a": {"type": "terms", "field": "kw8", "aggs": {"s": {"type": "stats", "field": "frac"}}}},
    "terms3000_global": {"a": {"type": "terms", "field": "kw3000", "missing": "none",
                               "aggs": {"s": {"type": "stats", "field": "frac"}}}},
    "cardinality": {"c": {"type": "cardinality", "field": "num"}, "s": {"type": "stats", "field": "num", "missing": 3}},
}


@pytest.mark.parametrize("name", list(REQUESTS))
@pytest.mark.parametrize("k", [0, 11])
def test_aggregations_over_the_scanned_docs(B, name, k):
    from searchlite_amd import aggs as AG
    from tests.test_gpu_agg_values import check_value_tables
    from tests.test_gpu_aggs import KEYS_OF
    request = REQUESTS[name]
    queries = [B.named(q) for q in (MA, CS(filter="third"), RF("pop", modifier="log"), CS(filter="no1", boost=0.5),
                                    RF("pop", modifier="reciprocal", boost=-1.0))]
    qf = np.array([-1, B.flt["no1"], -1, -1, B.flt["third"]], np.int32)
    _, want, matched, per_q = B.want(queries, k, qf)
    docs = [list(zip(sg.tolist(), dc.tolist())) for sg, dc, _ in per_q]
    assert all(s != 1 for s, _ in docs[1]) and any(s == 1 for s, _ in docs[0]), "a segment without a passing doc"
    plan = AG.agg_spec(request, B.fields)
    with B.ix.prepare_scan(queries, k, aggs=plan, q_filter=qf) as b:
        assert b.agg_layout()  # (before the first run)
        for again in range(2):
            b.run()
            same(b.fetch(), want, f"{name} k={k} rows")
            assert b.matched_counts().tolist() == matched.tolist()
            check_value_tables(plan, request, B.cols, docs, b.aggs(), b.agg_layout(), f"{name} k={k} run {again}", KEYS_OF)
    sort = [("low", "desc")]
    got = B.ix.search_scan(queries, k, sort=[(B.sort_id["low"], "desc")], aggs=plan, q_filter=qf)
    check_sorted(got[:5], sorted_rows(B, queries, sort, qf), k, sort, f"{name} sorted k={k}")
    check_value_tables(plan, request, B.cols, docs, got[5], got[6], f"{name} sorted k={k}", KEYS_OF)


# ---- lifecycle ---------------------------------------------------------------------------------------------
def test_run_twice_and_two_batches_in_flight(A, B):
    import torch
    qa = [A.named(q) for q in KINDS]
    want_a, matched_a = A.want(qa, 257)[1:3]
    b = A.ix.prepare_scan(qa, 257)
    for _ in range(2):
        b.run()
        same(b.fetch(), want_a, "run again")
        assert b.matched_counts().tolist() == matched_a.tolist()
    b.close()
    specs = [([MA, CS(filter="third", boost=2.0)], 11), ([RF("pop", modifier="log1p"), CS(filter="no1")], 300)]
    wants = [B.want(q, k) for q, k in specs]
    streams = [torch.cuda.Stream() for _ in specs]
    batches = [B.ix.prepare_scan(w[0], k) for w, (_, k) in zip(wants, specs)]
    for bb, s in zip(batches, streams):
        bb.set_stream(s.cuda_stream)
    for _ in range(3):
        for bb in batches:
            bb.run()
    for bb, w in zip(batches, wants):
        bb.sync()
        same(bb.fetch(), w[1], "in flight")
        assert bb.matched_counts().tolist() == w[2].tolist()
        bb.close()


def test_batch_keeps_its_index_state():
    """a batch prepared before slg_index_update_deleted answers against the state it was prepared on"""
    import searchlite_amd as sa
    rng = np.random.default_rng(71)
    sizes = [300, 2100]
    Wd = World(sa, sizes, [rng.random(300) < 0.1, None], tuning={"updatable": 1})
    try:
        Wd.add_field("v", [[[float(rng.integers(1, 100))] for _ in range(n)] for n in sizes], np.float64)
        Wd.add_filter("half", [rng.random(n) < 0.5 for n in sizes])
        queries = [MA, CS(filter="half", boost=2.0), RF("v", modifier="sqrt")]
        named, want_old, matched_old, _ = Wd.want(queries, 33)
        b = Wd.ix.prepare_scan(named, 33)
        dead = rng.random(2100) < 0.3
        Wd.ix.update_deleted(1, np.packbits(dead, bitorder="little"), 2100.0 - float(dead.sum()))
        b.run()
        same(b.fetch(), want_old, "prepared before the update")
        assert b.matched_counts().tolist() == matched_old.tolist()
        b.close()
        Wd.ref["deleted"][1] = dead
        # (a filter's bitmap holds deleted | ~filter of the state it is read in)
        _, matched_new, _ = Wd.check(queries, 33, "prepared after the update")
        assert (matched_new < matched_old).all()
        # a segment added after a field and a filter were registered: they have no column / bitmap for it
        from searchlite_amd import _native as N
        assert Wd.ix.add_segment(bare_segment(50)) == 2
        Wd.ref["n_docs"].append(50)
        Wd.ref["deleted"].append(None)
        for q, word in ((RF("v"), "no column for segment 2"), (CS(filter="half"), "unknown filter id")):
            with pytest.raises(N.SlgError) as ei:
                Wd.ix.prepare_scan([Wd.named(q)], 33)
            assert ei.value.code == N.ERR_INVALID and word in ei.value.msg, q
        with pytest.raises(N.SlgError) as ei:
            Wd.ix.prepare_scan([MA], 33, q_filter=[Wd.flt["half"]])
        assert ei.value.code == N.ERR_INVALID and "unknown filter id" in ei.value.msg
        _, matched_all, _ = Wd.check([MA], 33, "a segment added later")
        assert matched_all[0] == matched_new[0] + 50
    finally:
        Wd.ix.close()


def test_one_call_form_and_refusals(B):
    from searchlite_amd import _native as N, aggs as AG, scan, searcher
    from tests.test_gpu_agg_values import check_value_tables
    from tests.test_gpu_aggs import KEYS_OF
    k = 11
    queries = [B.named(q) for q in (MA, CS(filter="third", boost=2.0), RF("pop", modifier="log1p"))]
    nq = len(queries)
    spec, keep = scan.scan_spec(queries)
    _, want, matched, per_q = B.want(queries, k)
    lib, h = B.ix._lib, B.ix._h
    outs = [np.zeros((nq, k), dt) for dt in (np.uint32, np.uint32, F32)] + [np.zeros(nq, np.uint32)]
    got_matched = np.zeros(nq, np.uint64)
    N.check(lib.slg_search_batch_scan(h, nq, C.addressof(spec), None, None, None, k, *[a.ctypes.data for a in outs],
                                      got_matched.ctypes.data, None, None, None))
    same(tuple(outs), want, "one call")
    assert got_matched.tolist() == matched.tolist()
    # with aggregations: the outputs of slg_search_batch_agg_values
    request = REQUESTS["cardinality"]
    plan = AG.agg_spec(request, B.fields)
    with B.ix.prepare_scan(queries, k, aggs=plan) as b:
        b.run()
        tables, layout = b.aggs(), b.agg_layout()
    counts, stats, values = np.zeros((nq, 1), np.uint64), np.zeros((nq, 1), AG.STATS_DTYPE), np.zeros((nq, 1), np.uint64)
    N.check(lib.slg_search_batch_scan(h, nq, C.addressof(spec), None, None, C.addressof(plan.spec), k,
                                      *[a.ctypes.data for a in outs], None, counts.ctypes.data, stats.ctypes.data,
                                      values.ctypes.data))
    same(tuple(outs), want, "one call with aggregations")
    assert values[:, 0].tolist() == tables[0][:, 0, 0].tolist() and np.array_equal(stats[:, 0], tables[1][:, 0, 0])
    check_value_tables(plan, request, B.cols, [list(zip(sg.tolist(), dc.tolist())) for sg, dc, _ in per_q], tables, layout,
                       "one call", KEYS_OF)
    # a scan batch does not run sharded
    b = B.ix.prepare_scan(queries, k)
    try:
        group = searcher.ShardGroup(B.ix, 0, 1, searcher.shard_unique_id(), 3)
        try:
            for call in (lambda: b.run_sharded(group), b.fetch_sharded):
                with pytest.raises(N.SlgError) as ei:
                    call()
                assert ei.value.code == N.ERR_UNSUPPORTED and "scan batch" in ei.value.msg
        finally:
            group.close()
        with pytest.raises(N.SlgError):  # before the first run
            b.matched_counts()
    finally:
        b.close()
    # ids are checked against the batch's index state, before any device work
    kw = B.fields["kw8"]["id"]
    nonfin = B.ix.add_agg_field([[[math.inf]] * n for n in B.sizes], np.float64)
    late = B.ix.add_filter([np.ones(n, bool) for n in B.sizes])
    B.ix.remove_filter(late)
    try:
        for q, qf, code, word in ((RF(12345), None, N.ERR_INVALID, "unknown agg field"), (RF(kw), None, N.ERR_INVALID, "keyword"),
                                  (RF(nonfin), None, N.ERR_UNSUPPORTED, "non-finite"), (CS(filter=77), None, N.ERR_INVALID, "unknown filter"),
                                  (CS(filter=late), None, N.ERR_INVALID, "unknown filter"), (MA, [late], N.ERR_INVALID, "unknown filter"),
                                  (CS(boost=math.nan), None, N.ERR_INVALID, "non-finite score"),
                                  (RF(B.F["pop"], missing=math.inf), None, N.ERR_INVALID, "non-finite missing"),
                                  (RF(B.F["pop"], modifier=9), None, N.ERR_INVALID, "unknown modifier")):
            with pytest.raises(N.SlgError) as ei:
                B.ix.prepare_scan([q], k, q_filter=qf)
            assert ei.value.code == code and word in ei.value.msg, q
        with pytest.raises(N.SlgError) as ei:
            B.ix.prepare_scan([MA], N.MAX_K + 1)
        assert ei.value.code == N.ERR_UNSUPPORTED
        with pytest.raises(N.SlgError) as ei:
            B.ix.prepare_scan([MA], k, sort=[(9999, "asc")])
        assert ei.value.code == N.ERR_INVALID and "unknown sort field" in ei.value.msg
        assert lib.slg_batch_prepare_scan(h, 1, None, None, None, None, k) is None and N.last_error_code() == N.ERR_INVALID
    finally:
        B.ix.remove_agg_field(nonfin)
    # an empty batch, and an index whose only segment matches nothing
    got = B.ix.search_scan([], k)
    assert got[0].shape == (0, k) and len(got[4]) == 0
    got = B.ix.search_scan([B.named(CS(filter="no1"))], k, q_filter=np.array([B.flt["no1"]], np.int32))
    assert got[4][0] > 0 and got[3][0] == k
