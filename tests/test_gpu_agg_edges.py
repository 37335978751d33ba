"""agg_kernel at the boundaries its own constants create: the LDS / global choice at exactly SLG_AGG_LDS_BYTES,
columns of one value per doc (the offs == nullptr path) and CSR offsets that do not start at 0, many values per
doc, many slices per query, the f64 edges of the stats cells, and the histogram / range edges where the host's
row range meets the device's bucket formula.

Conventions of tests/test_gpu_aggs.py: run_check / check_tables against tests/agg_ref.py; counts, min, max and
the layout exact; every column holds exactly summable values, so the sums are exact in any order."""
import math

import numpy as np
import pytest

from tests import agg_ref as R
from tests.test_gpu_aggs import docs_of, run_check, tombstoned
from tests.util import random_queries, random_segment

gpu_test = pytest.mark.gpu
KEYS = {n: [f"{n}_{i:04d}" for i in range(c)] for n, c in (("kw8192", 8192), ("kw8191", 8191), ("kw1024", 1024),
                                                          ("kw512", 512))}
KEYS8 = [f"k{i}" for i in range(8)]
for _n in ("many_kw", "dense_kw", "mixed_kw", "reb_kw"):
    KEYS[_n] = KEYS8
F64_COLS = ("frac", "dense_f", "mixed_f", "reb_f", "edge_f", "sub", "zeros", "huge", "hot")
P1000 = 2.0 ** 1000
TINY = 2.0 ** -1074


def lds_bytes(layout):
    return sum(x["parent_rows"] * x["rows"] * (32 if x["is_stats"] else 4) for x in layout)


def make_columns(rng, sizes):
    """every column of the module, per segment per doc a list of values (strings for keyword fields)"""
    cols = {}

    def col(name, fn):
        cols[name] = [[fn(s, d) for d in range(n)] for s, n in enumerate(sizes)]

    ints = lambda lo, hi, n: [int(x) for x in rng.integers(lo, hi, n)]
    for name in ("kw8192", "kw8191", "kw1024", "kw512"):
        keys = KEYS[name]
        col(name, lambda s, d: [keys[j] for j in ints(0, len(keys), int(rng.integers(0, 3)))])
    # hnum: 0 .. 3583, both ends present: a histogram of interval 1 has exactly 3584 rows
    col("hnum", lambda s, d: ints(0, 3584, int(rng.integers(0, 3))))
    cols["hnum"][0][0], cols["hnum"][1][0] = [0], [3583]
    col("num", lambda s, d: ints(-50, 51, int(rng.integers(0, 3))))
    col("frac", lambda s, d: [x / 1024.0 for x in ints(-(1 << 20), 1 << 20, int(rng.integers(0, 3)))])
    # exactly one value per doc in every segment
    col("dense_kw", lambda s, d: [KEYS8[int(rng.integers(0, 8))]])
    col("dense_f", lambda s, d: [int(rng.integers(-(1 << 20), 1 << 20)) / 1024.0])
    col("dense_i", lambda s, d: ints(-50, 51, 1))
    cols["dense_i"][0][:4] = [[-50], [50], [-20], [30]]  # (values equal to the hard bounds used below)
    # one value per doc in segment 0, CSR in segment 1
    col("mixed_kw", lambda s, d: [KEYS8[j] for j in ints(0, 8, 1 if s == 0 else int(rng.integers(0, 3)))])
    col("mixed_f", lambda s, d: [x / 1024.0 for x in ints(-4096, 4096, 1 if s == 0 else int(rng.integers(0, 3)))])
    # registered with offsets that start at 5 (reb_i: one value per doc as well)
    col("reb_kw", lambda s, d: [KEYS8[j] for j in ints(0, 8, int(rng.integers(0, 3)))])
    col("reb_f", lambda s, d: [x / 1024.0 for x in ints(-4096, 4096, int(rng.integers(0, 3)))])
    col("reb_i", lambda s, d: ints(-50, 51, 1))
    # 0-12 values per doc with repeats
    col("many_kw", lambda s, d: [KEYS8[j] for j in ints(0, 8, int(rng.integers(0, 13)))])
    col("many", lambda s, d: ints(0, 20, int(rng.integers(0, 13))))
    # multiples of 0.1 as the nearest doubles, on and around bucket edges of interval 0.1; negative ids
    col("edge_f", lambda s, d: [j * 0.1 for j in ints(-30, 31, int(rng.integers(0, 3)))])
    # stats edges
    col("sub", lambda s, d: [j * TINY for j in ints(-1000, 1001, int(rng.integers(0, 3)))])
    col("zeros", lambda s, d: [(0.0, -0.0)[j] for j in ints(0, 2, int(rng.integers(1, 3)))])
    col("huge", lambda s, d: [P1000, -P1000] * int(rng.integers(0, 3)))  # pairs that cancel inside the doc
    col("big_i", lambda s, d: [(1 << 53) + 2 * 1024 * int(rng.integers(0, 500))])  # 2^53 + 2 j, j = 1024 m: see below
    col("odd_i", lambda s, d: [(1 << 53) + 2 * j for j in ints(0, 40, int(rng.integers(0, 3)))])
    col("hot", lambda s, d: [0.5])
    return cols


def rebased(per_seg, dtype, to_value):
    """per segment (offsets + 5, five leading values no offset names + the values)"""
    out = []
    for seg in per_seg:
        offs = np.zeros(len(seg) + 1, np.uint32)
        offs[1:] = np.cumsum([len(d) for d in seg])
        vals = [to_value(v) for d in seg for v in d]
        out.append((offs + 5, np.array([to_value(None)] * 5 + vals, dtype)))
    return out


def register(ix, cols):
    fields = {}
    for name, per_seg in cols.items():
        if name in KEYS:
            ord_of = {k: i for i, k in enumerate(KEYS[name])}
            if name.startswith("reb_"):
                data = rebased(per_seg, np.uint32, lambda v: 7 if v is None else ord_of[v])
            else:
                data = [[np.array([ord_of[v] for v in d], np.uint32) for d in seg] for seg in per_seg]
            fields[name] = {"id": ix.add_agg_keyword_field(data, len(ord_of)), "keys": KEYS[name]}
        else:
            dt = np.float64 if name in F64_COLS else np.int64
            data = rebased(per_seg, dt, lambda v: 99 if v is None else v) if name.startswith("reb_") else per_seg
            fields[name] = {"id": ix.add_agg_field(data, dt)}
    return fields


def build_world():
    """two segments of 1500 and 900 docs (tombstones in the first), four queries of three terms: query 0 names the
    commonest terms and matches nearly every live doc"""
    rng = np.random.default_rng(4242)
    segs = [random_segment(rng, 1500, 30, 25, k1=0.9, b=0.4), random_segment(rng, 900, 30, 25, k1=0.9, b=0.4)]
    segs[0] = tombstoned(segs[0], rng, 0.05)
    offs, terms, w = random_queries(rng, 4, 3, 30, n_segs=2, weights=True)
    terms[0:3, :] = np.array([0, 1, 2], np.uint32)[:, None]
    return dict(segs=segs, offs=offs, terms=terms, w=w, cols=make_columns(rng, [1500, 900]), keys_of=KEYS)


@pytest.fixture(scope="module")
def world(oracle):
    import searchlite_amd as sa
    W = build_world()
    W["docs"] = docs_of(oracle.search_batch(W["segs"], W["offs"], W["terms"], W["w"], 2400, strategy=oracle.BM25))
    W["ix"] = sa.GpuIndex(W["segs"])
    W["fields"] = register(W["ix"], W["cols"])
    yield W
    W["ix"].close()


# ---- 1. the LDS boundary ------------------------------------------------------------------------------------------
T_STATS = lambda kw: {"type": "terms", "field": kw, "aggs": {"s": {"type": "stats", "field": "frac"}}}
HIST1 = {"type": "histogram", "field": "hnum", "interval": 1}
LDS_CASES = {  # name: (request, bytes, on the LDS side)
    "terms8192": ({"a": {"type": "terms", "field": "kw8192"}}, 32768, True),
    "terms8192_missing_row": ({"a": {"type": "terms", "field": "kw8192", "missing": "none"}}, 32772, False),
    "terms8191": ({"a": {"type": "terms", "field": "kw8191"}}, 32764, True),
    "terms1024_stats": ({"t": T_STATS("kw1024")}, 4096 + 32768, False),
    # 512 x 4 + 512 x 32 = 18432, and 3584 histogram rows x 4 = 14336: 32768
    "terms512_stats_hist3584": ({"h": HIST1, "t": T_STATS("kw512")}, 32768, True),
    "terms512_stats_hist3585": ({"h": dict(HIST1, missing=3584), "t": T_STATS("kw512")}, 32772, False),
}
_lds_tables = {}


@gpu_test
@pytest.mark.parametrize("name", list(LDS_CASES))
def test_lds_boundary(world, name):
    from searchlite_amd import _native as N
    request, size, on_lds = LDS_CASES[name]
    plan, tables, layout = run_check(world, request, what=name)
    assert lds_bytes(layout) == size and (size <= N.AGG_LDS_BYTES) == on_lds, (name, lds_bytes(layout))
    assert sum(int(t["count"].sum()) if t.dtype.names else int(t.sum()) for t in tables) > 0
    _lds_tables[name] = tables
    # two specs that differ only by the side of the line: the cells they share are equal
    for a, b, rows in (("terms8192", "terms8192_missing_row", 8192), ("terms512_stats_hist3584", "terms512_stats_hist3585", 3584)):
        if a in _lds_tables and b in _lds_tables and name in (a, b):
            assert np.array_equal(_lds_tables[a][0], _lds_tables[b][0][:, :, :rows])
            for ta, tb in zip(_lds_tables[a][1:], _lds_tables[b][1:]):
                assert ta.tobytes() == tb.tobytes()


# ---- 2. one value per doc, and offsets that start at 5 ---------------------------------------------------------
def node_of(col):
    if col in KEYS:
        return [{"type": "terms", "field": col}]
    return [{"type": "histogram", "field": col, "interval": 16}, {"type": "stats", "field": col},
            {"type": "range", "field": col, "ranges": [{"to": 0}, {"from": 0, "to": 25}, {"from": -10}]}]


def root_and_children(col):
    """the column's nodes as roots and as children of a terms, a histogram and a range parent"""
    kids = {f"c{i}": n for i, n in enumerate(node_of(col))}
    parents = {"p_terms": {"type": "terms", "field": "many_kw", "missing": "none"},
               "p_hist": {"type": "histogram", "field": "many", "interval": 5},
               "p_range": {"type": "range", "field": "many", "ranges": [{"to": 4}, {"from": 4, "to": 12}, {"from": 10}]}}
    reqs = [{f"r{i}": n for i, n in enumerate(node_of(col))}]
    reqs += [{name: dict(body, aggs=kids)} for name, body in parents.items()]
    return reqs


DENSE_COLS = ("dense_kw", "dense_f", "dense_i", "mixed_kw", "mixed_f", "reb_kw", "reb_f", "reb_i")


def test_dense_columns_are_dense():
    """(no device) the columns meant for the one-value-per-doc path have one value per doc; the others do not"""
    cols = build_world()["cols"]
    one = lambda seg: all(len(d) == 1 for d in seg)
    for name in ("dense_kw", "dense_f", "dense_i", "reb_i", "hot", "big_i"):
        assert all(one(seg) for seg in cols[name]), name
    for name in ("mixed_kw", "mixed_f"):
        assert one(cols[name][0]) and not one(cols[name][1]), name
    for name in ("reb_kw", "reb_f", "many", "many_kw", "num"):
        assert not any(one(seg) for seg in cols[name]), name
    assert max(len(d) for seg in cols["many"] for d in seg) == 12 and max(len(d) for d in cols["many_kw"][0]) == 12
    assert rebased(cols["reb_i"], np.int64, lambda v: 99 if v is None else v)[0][0][0] == 5


@gpu_test
@pytest.mark.parametrize("col", DENSE_COLS)
def test_dense_and_rebased_columns(world, col):
    for i, request in enumerate(root_and_children(col)):
        plan, tables, layout = run_check(world, request, what=f"{col} request {i}")
        assert all(int(t["count"].sum()) if t.dtype.names else int(t.sum()) for t in tables), "every table counted docs"
    if col in ("dense_kw", "dense_i"):  # one value per doc: every matched doc is in exactly one root bucket
        plan, tables, layout = run_check(world, {"r": node_of(col)[0]}, what=col)
        assert tables[0].sum(axis=(1, 2)).tolist() == [len(d) for d in world["docs"]]


# ---- 3. many values per doc -----------------------------------------------------------------------------------
MANY = {"t": {"type": "terms", "field": "many_kw", "aggs": {"h": {"type": "histogram", "field": "many", "interval": 5}}},
        "h": {"type": "histogram", "field": "many", "interval": 5,  # (two values in one bucket count once)
              "aggs": {"t": {"type": "terms", "field": "many_kw", "missing": "k2"}}},
        "r": {"type": "range", "field": "many", "ranges": [{"to": 3}, {"from": 3, "to": 3}, {"from": 19}, {"from": 25}],
              "aggs": {"s": {"type": "stats", "field": "many"}}}}


@gpu_test
def test_many_values_per_doc(world):
    plan, tables, layout = run_check(world, MANY, what="0-12 values per doc")
    docs = world["docs"][0]
    n_values = sum(len(world["cols"]["many"][s][d]) for s, d in docs)
    assert int(tables[0].sum(axis=(1, 2))[0]) < n_values, "repeats in a bucket count once"


# ---- 4. many slices -------------------------------------------------------------------------------------------------
@gpu_test
def test_ten_segments_one_dead_one_filter(oracle):
    """ten segments of 60 docs, segment 4 fully tombstoned: a query has at least nine slices, so a wave of the slice
    loop takes three turns; half of the queries carry a filter"""
    import searchlite_amd as sa
    rng = np.random.default_rng(99)
    segs = [random_segment(rng, 60, 20, 10, k1=0.9, b=0.4) for _ in range(10)]
    segs[4] = tombstoned(segs[4], rng, 2.0)
    segs[7] = tombstoned(segs[7], rng, 0.3)
    assert segs[4].docs == 0.0
    offs, terms, w = random_queries(rng, 6, 3, 20, n_segs=10, weights=True)
    cols = {"many_kw": [[[KEYS8[j] for j in rng.integers(0, 8, int(rng.integers(0, 4)))] for _ in range(60)] for _ in segs],
            "num": [[[int(x) for x in rng.integers(-50, 51, int(rng.integers(0, 3)))] for _ in range(60)] for _ in segs]}
    masks = [rng.random(60) < 0.6 for _ in segs]
    req = {"t": {"type": "terms", "field": "many_kw", "missing": "none",
                 "aggs": {"s": {"type": "stats", "field": "num"}, "h": {"type": "histogram", "field": "num", "interval": 20}}}}
    with sa.GpuIndex(segs) as ix:
        fid = ix.add_filter(masks)
        qf = np.where(np.arange(6) % 2 == 0, fid, -1).astype(np.int32)
        want = oracle.search_batch_filtered(segs, offs, terms, w, 600, qf, {fid: masks}, strategy=oracle.BM25)
        W = dict(ix=ix, segs=segs, offs=offs, terms=terms, w=w, cols=cols, keys_of=KEYS, docs=docs_of(want),
                 fields=register(ix, cols))
        plan, tables, layout = run_check(W, req, what="ten segments", q_filter=qf)
        for d in W["docs"]:
            assert len({s for s, _ in d}) == 9 and 4 not in {s for s, _ in d}, "docs of nine segments"


# ---- 5. f64 edges of the stats cells ----------------------------------------------------------------------------
STATS_EDGES = ("sub", "zeros", "huge", "big_i", "hot")


@gpu_test
@pytest.mark.parametrize("col", STATS_EDGES)
def test_stats_f64_edges(world, col):
    """sub: multiples of 2^-1074 (a flush to zero in the atomic unit would change sum, min or max); zeros: +-0.0;
    huge: +-2^1000 in pairs (partial sums are multiples of 2^1000 below 2^1012: exact); big_i: 2^53 + 2 j with
    j = 1024 m, so multiples of 2048 below 2^54, summed per bucket of a sparse terms parent (at most 8 values: the
    partial sums stay below 2^57, where the spacing is 16); hot: 0.5 in every doc, one cell that every thread
    hits."""
    request = {"s": {"type": "stats", "field": col},
               "t": {"type": "terms", "field": "dense_kw", "aggs": {"s": {"type": "stats", "field": col}}}}
    if col == "big_i":  # (a root sum of 2300 values near 2^53 is not exact in every order)
        request = {"t": {"type": "terms", "field": "kw8192", "aggs": {"s": {"type": "stats", "field": col}}}}
    plan, tables, layout = run_check(world, request, what=col)
    root = tables[0][:, 0, 0] if col != "big_i" else None
    if col == "sub":
        assert (np.abs(root["min"]) < 2.0 ** -1022).all() and (root["min"] < 0).all() and (root["max"] > 0).all()
    if col == "zeros":
        assert (root["min"] == 0).all() and (root["max"] == 0).all() and (root["sum"] == 0).all() and (root["count"] > 0).all()
        print("signs of zero (min, max, sum):", np.signbit(root["min"]).tolist(), np.signbit(root["max"]).tolist(),
              np.signbit(root["sum"]).tolist())
    if col == "huge":
        assert (root["sum"] == 0).all() and (root["max"] == P1000).all() and (root["min"] == -P1000).all()
    if col == "big_i":
        cell = tables[1][:, :, 0]
        assert int(cell["count"].max()) <= 8, "few docs per bucket: at most 8 values of < 2^54, multiples of 2048"
        assert (cell["max"][cell["count"] > 0] >= 2.0 ** 53).all()
    if col == "hot":
        assert int(root["count"][0]) == len(world["docs"][0]) >= 2000
        assert root["sum"][0] == 0.5 * len(world["docs"][0]) and root["min"][0] == root["max"][0] == 0.5


@gpu_test
def test_i64_beyond_2_53_keeps_even_values_apart(world):
    """odd_i = 2^53 + 2 j: a histogram of interval 2 from 2^53 puts value j into bucket j, a range [v, v] holds
    exactly the docs with v"""
    v = lambda j: float((1 << 53) + 2 * j)
    request = {"h": {"type": "histogram", "field": "odd_i", "interval": 2, "offset": v(0)},
               "r": {"type": "range", "field": "odd_i", "ranges": [{"from": v(j), "to": v(j)} for j in (0, 1, 20, 39, 40)]}}
    plan, tables, layout = run_check(world, request, what="odd_i")
    assert (layout[0]["first_id"], layout[0]["rows"]) == (0, 40)
    assert np.array_equal(tables[1][:, 0, :4], tables[0][:, 0, [0, 1, 20, 39]]) and not tables[1][:, 0, 4].any()


# ---- 6. histogram and range edges -------------------------------------------------------------------------------
INF = math.inf
HIST_RANGE = {  # name: (request, (first_id, rows) of node 0 or None)
    "interval_0.1_on_bucket_edges": ({"h": {"type": "histogram", "field": "edge_f", "interval": 0.1}}, None),
    "interval_0.1_offset": ({"h": {"type": "histogram", "field": "edge_f", "interval": 0.1, "offset": 0.05,
                                   "aggs": {"s": {"type": "stats", "field": "frac"}}}}, None),
    "negative_first_id": ({"h": {"type": "histogram", "field": "dense_i", "interval": 7, "offset": 3}}, (-8, 15)),
    "missing_above_the_column": ({"h": {"type": "histogram", "field": "num", "interval": 10, "missing": 500}}, (-5, 56)),
    "missing_below_the_column": ({"h": {"type": "histogram", "field": "num", "interval": 10, "missing": -500.5}}, (-51, 57)),
    "hard_bounds_equal_to_values": ({"h": {"type": "histogram", "field": "dense_i", "interval": 10,
                                           "hard_bounds": {"min": -20, "max": 30}}}, (-2, 6)),
    "hard_bounds_exclude_everything": ({"h": {"type": "histogram", "field": "dense_i", "interval": 10,
                                              "hard_bounds": {"min": 1000, "max": 2000}}}, (0, 1)),
    "hard_bounds_exclude_missing": ({"h": {"type": "histogram", "field": "num", "interval": 10, "missing": 500,
                                           "hard_bounds": {"min": -50, "max": 50}}}, (-5, 11)),
    "sixteen_ranges": ({"r": {"type": "range", "field": "num", "missing": 0, "ranges":
                              [{"from": -50 + 6 * i, "to": -44 + 6 * i} for i in range(12)] +
                              [{"from": 10, "to": -10}, {"from": -INF, "to": INF}, {"from": -INF, "to": 0}, {"from": 50}],
                              "aggs": {"s": {"type": "stats", "field": "num"}}}}, None),
    "all_ranges_overlap": ({"r": {"type": "range", "field": "many",
                                  "ranges": [{"from": i, "to": 19 - i} for i in range(8)]}}, None),
}


@pytest.mark.parametrize("name", list(HIST_RANGE))
def test_histogram_layouts_of_the_reference(name):
    """(no device) the rows and first id agg_ref gives each histogram above, derived by hand: dense_i spans -50 ..
    50, num spans -50 .. 50, edge_f spans -3.0 .. 3.0"""
    from searchlite_amd import aggs as A
    request, want = HIST_RANGE[name]
    W = _cpu_world()
    fields = {n: {"id": i, "keys": KEYS.get(n)} for i, n in enumerate(W["cols"])}
    plan = A.agg_spec(request, fields)
    lay = R.ref_layout(plan.nodes, W["cols"], KEYS)
    if want is not None:
        assert (lay[0]["first_id"], lay[0]["rows"]) == want
    if name.startswith("interval_0.1"):
        off = request["h"].get("offset", 0.0)
        assert lay[0]["first_id"] == math.floor((-30 * 0.1 - off) / 0.1) < 0
        # the nearest doubles of j / 10 fall on either side of the quotient's edge: ids are not simply j
        ids = [R.bucket_id(j * 0.1, 0.1, 0.0) for j in range(-30, 31)]
        assert any(i != j for i, j in zip(ids, range(-30, 31)))
    if name == "sixteen_ranges":
        from searchlite_amd import _native as N
        assert plan.spec.nodes[0].n_ranges == N.MAX_AGG_RANGES == 16


_cpu = {}


def _cpu_world():
    if not _cpu:
        _cpu.update(build_world())
    return _cpu


@gpu_test
@pytest.mark.parametrize("name", list(HIST_RANGE))
def test_histogram_and_range_edges(world, name):
    request, want = HIST_RANGE[name]
    plan, tables, layout = run_check(world, request, what=name)
    if want is not None:
        assert (layout[0]["first_id"], layout[0]["rows"]) == want
    counted = int(tables[0].sum())
    if name == "hard_bounds_exclude_everything":
        assert counted == 0
    else:
        assert counted > 0
    if name == "hard_bounds_equal_to_values":  # -20 and 30 are values of docs (0, 2) and (0, 3): first and last row
        assert tables[0][0, 0, 0] > 0 and tables[0][0, 0, -1] > 0
    if name == "sixteen_ranges":
        assert not tables[0][:, 0, 12].any(), "from > to holds nothing"
        assert tables[0][:, 0, 13].tolist() == [len(d) for d in world["docs"]], "(-inf, inf) with missing holds every doc"
    if name == "all_ranges_overlap":
        assert (np.diff(tables[0][:, 0, :].astype(np.int64), axis=1) <= 0).all() and tables[0][0, 0, 7] > 0


@gpu_test
def test_histogram_refusals(world):
    """bucket ids beyond 9e15 and more than SLG_MAX_AGG_CELLS buckets are refused before any launch; a valid
    batch afterwards is right"""
    from searchlite_amd import _native as N, aggs as A
    W = world
    for request in ({"h": {"type": "histogram", "field": "huge", "interval": 1}},              # ids of +-2^1000
                    {"h": {"type": "histogram", "field": "odd_i", "interval": 1, "offset": -1e15}},  # ids above 9e15
                    {"h": {"type": "histogram", "field": "hnum", "interval": 0.05}},           # 71 680 buckets
                    {"h": {"type": "histogram", "field": "num", "interval": 1, "missing": 65500}}):  # 65 551 buckets
        with pytest.raises(N.SlgError) as ei:
            W["ix"].search_aggs(W["offs"], W["terms"], W["w"], 11, A.agg_spec(request, W["fields"]))
        assert ei.value.code == N.ERR_UNSUPPORTED, request
    plan, tables, layout = run_check(W, {"h": {"type": "histogram", "field": "hnum", "interval": 0.0547}}, what="65 503 buckets")
    assert 65000 < layout[0]["rows"] <= N.MAX_AGG_CELLS
