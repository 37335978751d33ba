"""date_histogram, filter, date_range and value_count aggregations on the device (SLG_AGG_DATE_HISTOGRAM,
SLG_AGG_FILTER; date_range and value_count through searchlite_amd.aggs onto the range and stats kinds).

The aggregated set of a query is what the oracle returns with k >= the number of docs; the expected tables and
responses are tests/agg_date_ref.py's collectors over that set (calendar arithmetic through datetime).  Bar: layout
(rows, first_id), counts, stats (the columns hold exactly summable values, so a sum is the same in every order: the
bound of a stats sum, 2 (n - 1) 2^-53 sum|x|, is held with zero error) and aggs.shape() equal to the helper; the
batch's rows bit-identical to the same batch without aggregations; matched = the size of the set.
"""
import copy
import json
import os

import numpy as np
import pytest

from tests import agg_date_ref as D
from tests.util import _append_lists, random_queries, random_segment

pytestmark = pytest.mark.gpu

NO_TERM = 0xFFFFFFFF
KEYS = [f"k{i}" for i in range(5)]
KEYS_OF = {"kw": KEYS}
DAY, HOUR = 86_400_000, 3_600_000
VOCAB = 40
ISO = lambda ms: (D.EPOCH + ms * D.MS).strftime("%Y-%m-%dT%H:%M:%S.") + f"{ms % 1000:03d}Z"


def make_world(rng):
    """Plain data, no device.  Two segments of 210 and 190 docs (more than 64 candidates per slice: the lane loop of
    agg_walk goes round); term VOCAB is held by every doc.  Columns: kw keyword, 0-2 of 5 keys; x f64 multiples of
    0.25 in [-6, 6] (fractional and negative-fractional; exactly summable), 0-2 values; ts i64 timestamps drawn from
    the edge list (agg_date_ref.edge_instants): about 10 % of the docs have none, about 15 % have 2-3, some in one
    bucket (v, v + 1) and some in different ones; near i64 around second and day boundaries within +-30 days, 0-2
    values; n i64 in [0, 99], one value."""
    segs = []
    for n_docs in (210, 190):
        s = random_segment(rng, n_docs, VOCAB, 12, k1=0.9, b=0.4)
        segs.append(_append_lists(s, [(np.arange(n_docs), np.ones(n_docs))]))
    dead = rng.random(190) < 0.1
    segs[1].deleted = np.packbits(dead, bitorder="little")
    segs[1].docs = float(190 - int(dead.sum()))
    edges = D.edge_instants()
    inner = [v for v in edges if D.MIN_MS < v < D.MAX_MS - 1]
    near_pool = [k * 1000 + d for k in range(-3, 4) for d in (-1, 0, 1, 499, 500, 501)] + \
        [k * DAY + d for k in range(-30, 31) for d in (-4, -3, -2, -1, 0, 1, 499, 500, 501)]
    cols = {n: [] for n in ("kw", "x", "ts", "near", "n")}
    for s in segs:
        ts = []
        for _ in range(s.n_docs):
            r = rng.random()
            if r < 0.10:
                ts.append([])
            elif r < 0.18:  # two values in one bucket of every unit (and of no 1 ms step)
                v = int(rng.choice(inner))
                ts.append([v, v + 1] if D.day_of(v) == D.day_of(v + 1) else [v, v - 1])
            elif r < 0.25:
                ts.append([int(v) for v in rng.choice(edges, int(rng.integers(2, 4)))])
            else:
                ts.append([int(rng.choice(edges))])
        cols["ts"].append(ts)
        cols["kw"].append([[KEYS[j] for j in rng.integers(0, 5, int(rng.integers(0, 3)))] for _ in range(s.n_docs)])
        cols["x"].append([[float(v) / 4.0 for v in rng.integers(-24, 25, int(rng.integers(0, 3)))]
                          for _ in range(s.n_docs)])
        cols["near"].append([[int(v) for v in rng.choice(near_pool, int(rng.integers(0, 3)))] for _ in range(s.n_docs)])
        cols["n"].append([[int(rng.integers(0, 100))] for _ in range(s.n_docs)])
    flat = [v for seg in cols["x"] for d in seg for v in d]
    assert -0.5 in flat and -1.5 in flat and any(v > 0 and v != int(v) for v in flat)
    assert {D.MIN_MS, D.MAX_MS, 0, -1} <= {v for seg in cols["ts"] for d in seg for v in d}
    # a handful of term queries over subsets, one query that matches every doc, one that matches none
    offs, terms, w = random_queries(rng, 8, 2, VOCAB, n_segs=2, weights=True)
    terms[12:14, :] = [[VOCAB, VOCAB], [NO_TERM, NO_TERM]]
    terms[14:16, :] = NO_TERM
    masks = {"odd": [np.arange(s.n_docs) % 2 == 1 for s in segs], "third": [rng.random(s.n_docs) < 0.33 for s in segs],
             "half": [rng.random(s.n_docs) < 0.5 for s in segs]}
    tree = {"I64Range": {"field": "n", "min": 20, "max": 59}}
    masks["tree"] = [np.array([20 <= d[0] <= 59 for d in seg]) for seg in cols["n"]]
    return dict(segs=segs, cols=cols, offs=offs, terms=terms, w=w, masks=masks, tree=tree,
                k_all=sum(s.n_docs for s in segs))


def docs_of(hits):
    doc, seg, _, count = hits
    return [[(int(seg[q, i]), int(doc[q, i])) for i in range(int(count[q]))] for q in range(len(count))]


def register(ix, W):
    """the columns, the bitmap filters and the filter tree -> the `fields` map of aggs.agg_spec"""
    from searchlite_amd import aggs as A, filters
    cols = W["cols"]
    ord_of = {k: i for i, k in enumerate(KEYS)}
    fields = {"kw": {"id": ix.add_agg_keyword_field([[np.array([ord_of[v] for v in d], np.uint32) for d in seg]
                                                     for seg in cols["kw"]], len(KEYS)), "keys": KEYS},
              "x": {"id": ix.add_agg_field(cols["x"], np.float64)}}
    for name in ("ts", "near", "n"):
        fields[name] = {"id": ix.add_agg_field(cols[name], np.int64)}
    ids = {name: ix.add_filter(W["masks"][name]) for name in ("odd", "third", "half")}
    prog = filters.compile_filter(W["tree"], {"n": dict(id=fields["n"]["id"], kind="i64")})
    ids["tree"] = ix.add_filter_trees([prog])[0]
    fields[A.FILTERS] = lambda body: ids[body["name"]]
    return fields, ids


@pytest.fixture(scope="module")
def world(oracle):
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    W = make_world(np.random.default_rng(20240229))
    W["ix"] = sa.GpuIndex(W["segs"])
    W["fields"], W["filter_ids"] = register(W["ix"], W)
    W["ix"].rank_agg_field(W["fields"]["near"]["id"])
    W["sort"] = [(W["ix"].add_sort_field(W["cols"]["n"], np.int64), "asc"), ("_score", "desc")]
    W["docs"] = docs_of(oracle.search_batch(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], strategy=oracle.BM25))
    assert len(W["docs"][6]) == 210 + int(W["segs"][1].docs) and W["docs"][7] == [] and max(map(len, W["docs"][:6])) > 64
    yield W
    W["ix"].close()


def planned(request, fields):
    """agg_spec, with what a request's strings cannot say: body["_override"] = {"offset": ms} (a negative offset)"""
    from searchlite_amd import aggs as A
    plan = A.agg_spec(request, fields)
    for i, nd in enumerate(plan.nodes):
        over = nd["body"].get("_override")
        if over:
            nd["date"].update(over)
            plan.spec.nodes[i].date_offset = nd["date"]["offset"]
    return plan


_expected = {}


def expected(W, request, plan, docs, key, resp_q=None):
    """the helper's layout, tables and responses of every query, once per (request, doc sets).  resp_q: the queries
    whose response is compared (None: all; the walk over the zero buckets of a table of tens of thousands of rows
    takes a second per query here, so the tests of the global home name the query that matches every doc)"""
    if key is not None and key in _expected:
        return _expected[key]
    passes = W["masks"]
    layout = D.ref_layout(plan.nodes, W["cols"], KEYS_OF)
    states = [D.run(request, W["cols"], passes, d) for d in docs]
    per_q = [D.dense(plan.nodes, layout, st, KEYS_OF) for st in states]
    out = layout, [np.stack([t[i] for t in per_q]) for i in range(len(plan.nodes))], \
        {q: D.respond(request, states[q]) for q in (range(len(states)) if resp_q is None else resp_q)}
    if key is not None:
        _expected[key] = out
    return out


def check(plan, got_tables, got_layout, want, what):
    from searchlite_amd import aggs as A
    want_layout, want_tables, want_resp = want
    for i, (g, w) in enumerate(zip(got_tables, want_tables)):
        gl, wl = got_layout[i], want_layout[i]
        assert (gl["parent_rows"], gl["rows"], gl["first_id"]) == (wl["parent_rows"], wl["rows"], wl["first_id"]), \
            f"{what} node {i}: layout {gl} != {wl}"
        assert g.shape == w.shape, f"{what} node {i}: shape {g.shape} != {w.shape}"
        if gl["is_stats"]:
            for f in ("count", "min", "max", "sum"):  # (exactly summable values: see the module's docstring)
                assert np.array_equal(g[f], w[f]), f"{what} node {i}: stats {f} differ"
        else:
            assert np.array_equal(g, w), f"{what} node {i}: cells differ at {np.argwhere(g != w)[:5].tolist()}"
    for q, resp in want_resp.items():
        assert A.shape(plan, got_layout, got_tables, q) == resp, f"{what}: response of query {q}"


def run_check(W, request, sort=None, docs=None, key=None, what="", k=11, resp_q=None, **kw):
    """one aggregation batch against the helper and against the same batch without aggregations"""
    ix = W["ix"]
    plan = planned(request, W["fields"])
    docs = W["docs"] if docs is None else docs
    want = expected(W, request, plan, docs, key, resp_q)
    doc, seg, score, count, matched, tables, layout = ix.search_aggs(W["offs"], W["terms"], W["w"], k, plan, sort=sort, **kw)
    if sort is None:
        with ix.prepare(W["offs"], W["terms"], W["w"], k, **kw) as b:
            b.run()
            base = b.fetch()
    else:
        base = ix.search_sorted(W["offs"], W["terms"], W["w"], k, sort, **kw)
    for name, a, b_ in zip(("doc", "seg", "score", "count"), (doc, seg, score, count), base):
        assert np.array_equal(a.view(np.uint32), b_.view(np.uint32)), f"{what}: {name} rows differ from the plain batch"
    assert matched.tolist() == [len(d) for d in docs], f"{what}: matched"
    check(plan, tables, layout, want, what)
    return plan, tables, layout


def table_bytes(layout):
    return sum(x["parent_rows"] * x["rows"] * (32 if x["is_stats"] else 4) for x in layout)


# ---- 1, 13: the reference's recorded cases, end to end ------------------------------------------------------------
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agg_date_cases.json")) as fh:
    CASES = {c["name"]: c for c in json.load(fh)["cases"]}


@pytest.mark.parametrize("name", list(CASES))
def test_reference_recorded_cases(name):
    import searchlite_amd as sa
    from searchlite_amd import aggs as A
    from tests.test_agg_date_ref import check_expected, prepared
    case = CASES[name]
    req, passes = prepared(case)
    cols = case["columns"]
    n_docs = len(next(iter(cols.values()))[0])
    rng = np.random.default_rng(5)
    seg = _append_lists(random_segment(rng, n_docs, 5, 3, k1=0.9, b=0.4), [(np.arange(n_docs), np.ones(n_docs))])
    offs, terms, w = np.array([0, 1], np.uint32), np.array([[5]], np.uint32), np.ones(1, np.float32)
    with sa.GpuIndex([seg]) as ix:
        fields = {}
        for f, per_seg in cols.items():
            if isinstance(next((v for d in per_seg[0] for v in d), 0), str):
                keys = sorted({v for d in per_seg[0] for v in d})
                fields[f] = {"id": ix.add_agg_keyword_field([[np.array([keys.index(v) for v in d], np.uint32)
                                                              for d in per_seg[0]]], len(keys)), "keys": keys}
            else:
                fields[f] = {"id": ix.add_agg_field(per_seg, np.int64)}
        ids = {n: ix.add_filter([np.array(m[0], bool)]) for n, m in passes.items()}
        fields[A.FILTERS] = lambda body: ids[body["name"]]
        plan = A.agg_spec(req, fields)
        *_, matched, tables, layout = ix.search_aggs(offs, terms, w, 1, plan)  # (limit 1: aggregations see all docs)
        assert int(matched[0]) == n_docs
        got = A.shape(plan, layout, tables, 0)
    for agg, want in case["expected"].items():
        check_expected(got[agg], want, f"{name}.{agg}")
    assert got == D.respond(req, D.run(req, cols, passes, [(0, d) for d in range(n_docs)]))


# ---- 2: fixed steps and offsets ---------------------------------------------------------------------------------
FIXED_BOUNDS = {1: 3000, 7: 3000, 1000: 20000, 86_400_000: None}  # (hard bounds keep the dense range small)


@pytest.mark.parametrize("offset", [0, 500, -3])
@pytest.mark.parametrize("step", [1, 7, 1000, 86_400_000])
def test_fixed_steps_and_offsets(world, step, offset):
    body = {"type": "date_histogram", "field": "near", "fixed_interval": f"{step}ms", "_override": {"offset": offset},
            "aggs": {"s": {"type": "stats", "field": "x"}}}
    if FIXED_BOUNDS[step] is not None:
        body["hard_bounds"] = {"min": str(-FIXED_BOUNDS[step]), "max": str(FIXED_BOUNDS[step])}
    plan, tables, layout = run_check(world, {"h": body}, key=f"fixed {step} {offset}", what=f"fixed {step} {offset}")
    assert plan.spec.nodes[0].date_step == step and plan.spec.nodes[0].date_offset == offset
    assert tables[0].sum() > 0 and layout[0]["rows"] > 1


def test_fixed_step_on_an_f64_column_truncates_toward_zero(world):
    """`as i64`: -0.5 -> 0 and -1.5 -> -1; with a 1 ms step the bucket is the truncated value itself"""
    req = {"h": {"type": "date_histogram", "field": "x", "fixed_interval": "1ms"},
           "o": {"type": "date_histogram", "field": "x", "fixed_interval": "2ms", "offset": "1ms", "missing": 3.75}}
    plan, tables, layout = run_check(world, req, key="f64", what="f64 column")
    flat = [int(v) for seg in world["cols"]["x"] for d in seg for v in d]  # (int(): toward zero)
    assert (layout[0]["first_id"], layout[0]["rows"]) == (min(flat), max(flat) - min(flat) + 1) and min(flat) < 0 < max(flat)
    q, first = 6, layout[0]["first_id"]  # the query that matches every doc
    want0 = sum(1 for s, d in world["docs"][q] if any(-1.0 < v < 1.0 for v in world["cols"]["x"][s][d]))
    assert int(tables[0][q, 0, 0 - first]) == want0 and want0 > 0


# ---- 3: calendar units, both homes ------------------------------------------------------------------------------
CALENDAR = {
    "day_epoch": ("day", "1969-12-01T00:00:00Z", "1970-02-01T00:00:00Z"),
    "day_2024": ("1d", "2023-12-01T00:00:00Z", "2024-05-01T00:00:00Z"),
    "day_year_1": ("day", "0001-01-01T00:00:00Z", "0001-03-01T00:00:00Z"),
    "day_year_9999": ("day", "9999-11-01T00:00:00Z", "9999-12-31T23:59:59.999Z"),
    "week_epoch": ("week", "1969-12-01T00:00:00Z", "1970-02-01T00:00:00Z"),
    "week_1900": ("1w", "1900-01-01T00:00:00Z", "1900-04-01T00:00:00Z"),
    "week_2024": ("week", "2023-12-01T00:00:00Z", "2024-05-01T00:00:00Z"),
    "month_lds": ("month", "1900-01-01T00:00:00Z", "2024-12-31T23:59:59.999Z"),
    "month_global": ("1m", "1300-01-01T00:00:00Z", "2024-12-31T23:59:59.999Z"),
    "quarter_global": ("quarter", None, None),
    "year_global": ("year", None, None),
}


# (0001-01-01T00:00:00Z - 1 h would leave the supported range: test_refusals)
@pytest.mark.parametrize("name,offset", [(n, o) for n in CALENDAR for o in (None, "1h") if (n, o) != ("day_year_1", "1h")])
def test_calendar_units_in_both_homes(world, name, offset):
    from searchlite_amd import _native as N
    unit, lo, hi = CALENDAR[name]
    body = {"type": "date_histogram", "field": "ts", "calendar_interval": unit}
    if offset is not None:
        body["offset"] = offset
    if lo is None and offset is not None:
        lo, hi = "0001-01-01T01:00:00Z", "9999-12-31T23:59:59.999Z"
    if lo is not None:
        body["hard_bounds"] = {"min": lo, "max": hi}
    plan, tables, layout = run_check(world, {"h": body}, key=f"{name} {offset}", what=f"{name} offset {offset}",
                                     resp_q=(6,) if name.endswith("global") else None)
    assert tables[0][6].sum() > 0
    if name.endswith("global"):
        assert table_bytes(layout) > N.AGG_LDS_BYTES
        if name == "year_global" and offset is None:
            assert (layout[0]["first_id"], layout[0]["rows"]) == (1 - 1970, 9999)
    else:
        assert table_bytes(layout) <= N.AGG_LDS_BYTES
        if name == "month_lds":
            assert (layout[0]["first_id"], layout[0]["rows"]) == ((1900 - 1970) * 12 - (offset is not None), 1500 + (offset is not None))


# ---- 4, 5, 6: hard bounds, missing, a doc with two values in one bucket ---------------------------------------
def test_hard_bounds(world):
    ts = world["cols"]["ts"]
    leap = (D.datetime(2024, 2, 29) - D.EPOCH) // D.MS
    # inclusive at both ends: the bounds are values the column holds, 1 ms inside the neighbours it also holds
    assert all(any(v in d for seg in ts for d in seg) for v in (leap - 1, leap, leap + 1, -1, 0))
    both = {"type": "date_histogram", "field": "ts", "calendar_interval": "day",
            "hard_bounds": {"min": "-1", "max": ISO(leap)}, "aggs": {"s": {"type": "stats", "field": "x"}}}
    plan, tables, layout = run_check(world, {"h": both}, key="hard inclusive", what="inclusive bounds")
    first, rows = layout[0]["first_id"], layout[0]["rows"]
    assert (first, first + rows - 1) == (-1, leap // DAY)
    assert tables[0][6, 0, 0] > 0 and tables[0][6, 0, rows - 1] > 0  # the days of -1 ms and of the leap day's 00:00:00.000
    # a doc with one value inside and one outside counts inside only (the helper decides; such docs exist)
    inside = lambda v: -1 <= v <= leap
    assert any(len(d) > 1 and any(map(inside, d)) and not all(map(inside, d)) for seg in ts for d in seg)
    # bounds that leave nothing: outside every value (one row, never counted) and between the values
    none = {"type": "date_histogram", "field": "near", "fixed_interval": "1s", "missing": "7",
            "hard_bounds": {"min": "1000000000000", "max": "1000000000005"}, "aggs": {"t": {"type": "terms", "field": "kw"}}}
    plan, tables, layout = run_check(world, {"h": none}, key="hard nothing", what="bounds that leave nothing")
    assert (layout[0]["rows"], layout[1]["parent_rows"]) == (1, 1) and tables[0].sum() == 0 and tables[1].sum() == 0
    gap = dict(none, hard_bounds={"min": "5", "max": "6"}, fixed_interval="1ms")
    del gap["missing"]
    plan, tables, layout = run_check(world, {"h": gap}, key="hard gap", what="bounds between the values")
    assert layout[0]["rows"] == 2 and tables[0].sum() == 0


@pytest.mark.parametrize("missing", ["2000-02-29T12:00:00Z", 951_825_600_000, "951825600000.75", -0.5])
def test_missing_as_a_date_and_as_a_number(world, missing):
    req = {"h": {"type": "date_histogram", "field": "ts", "calendar_interval": "month", "missing": missing,
                 "hard_bounds": {"min": "1969-01-01T00:00:00Z", "max": "2001-01-01T00:00:00Z"}}}
    plan, tables, layout = run_check(world, req, key=f"missing {missing}", what=f"missing {missing}")
    ts = world["cols"]["ts"]
    no_value = sum(1 for s, d in world["docs"][6] if not ts[s][d])
    row = (0 if missing == -0.5 else (2000 - 1970) * 12 + 1) - layout[0]["first_id"]
    assert no_value > 0 and int(tables[0][6, 0, row]) >= no_value


def test_two_values_in_one_bucket_count_once(world):
    """docs with (v, v + 1) in one day: counted once, and the children collect once (stats count = the doc's x values)"""
    ts, x = world["cols"]["ts"], world["cols"]["x"]
    req = {"h": {"type": "date_histogram", "field": "ts", "calendar_interval": "year",
                 "aggs": {"s": {"type": "stats", "field": "x"}, "v": {"type": "value_count", "field": "x"}}}}
    plan, tables, layout = run_check(world, req, key="once", what="two values in one bucket")
    docs = world["docs"][6]
    twice = [(s, d) for s, d in docs if len(ts[s][d]) == 2 and abs(ts[s][d][0] - ts[s][d][1]) == 1]
    assert len(twice) > 5
    in_buckets = sum(len({D.day_of(v).year for v in ts[s][d]}) for s, d in docs)
    assert int(tables[0][6].sum()) == in_buckets < sum(len(ts[s][d]) for s, d in docs)
    assert int(tables[1][6]["count"].sum()) == sum(len({D.day_of(v).year for v in ts[s][d]}) * len(x[s][d]) for s, d in docs)
    assert np.array_equal(tables[1]["count"], tables[2]["count"])


# ---- 7: nesting -----------------------------------------------------------------------------------------------
BOUNDED = {"type": "date_histogram", "field": "ts", "calendar_interval": "quarter",
           "hard_bounds": {"min": "1969-01-01T00:00:00Z", "max": "2024-12-31T00:00:00Z"}}
NESTING = {
    "date_children": {"h": dict(BOUNDED, aggs={"s": {"type": "stats", "field": "x", "missing": 0.5},
                                               "t": {"type": "terms", "field": "kw", "missing": "none"},
                                               "c": {"type": "cardinality", "field": "kw"},
                                               "n": {"type": "cardinality", "field": "near", "missing": 3},
                                               "r": {"type": "percentile_ranks", "field": "x", "values": [-1.0, 0.0, 2.5]},
                                               "f": {"type": "filter", "filter": {"name": "third"}},
                                               "d": {"type": "date_range", "field": "ts",
                                                     "ranges": [{"to": "1970-01-01T00:00:00Z"}, {"from": "0"}]}})},
    "terms_date": {"t": {"type": "terms", "field": "kw", "missing": "none",
                         "aggs": {"h": dict(BOUNDED, calendar_interval="month", offset="1h"),
                                  "w": {"type": "date_histogram", "field": "near", "fixed_interval": "1w", "missing": 0}}}},
    "older_parents": {"g": {"type": "histogram", "field": "n", "interval": 25,
                            "aggs": {"h": dict(BOUNDED, calendar_interval="year"),
                                     "f": {"type": "filter", "filter": {"name": "tree"}}}},
                      "r": {"type": "range", "field": "x", "ranges": [{"to": 0}, {"from": 0}],
                            "aggs": {"f": {"type": "filter", "filter": {"name": "odd"}}}}},
    "filter_children": {"f": {"type": "filter", "filter": {"name": "half"},
                              "aggs": {"h": {"type": "date_histogram", "field": "ts", "calendar_interval": "year"},
                                       "s": {"type": "stats", "field": "x"},
                                       "c": {"type": "cardinality", "field": "kw", "missing": "k1"},
                                       "r": {"type": "percentile_ranks", "field": "near", "values": [0, 500]},
                                       "g": {"type": "filter", "filter": {"name": "odd"}},
                                       "t": {"type": "terms", "field": "kw"}}},
                        "p": {"type": "percentiles", "field": "near", "percents": [50.0]}},
    "two_root_filters": {"a": {"type": "filter", "filter": {"name": "odd"}},
                         "b": {"type": "filter", "filter": {"name": "tree"},
                               "aggs": {"s": {"type": "stats", "field": "x"}}},
                         "v": {"type": "value_count", "field": "ts", "missing": 1}},
}


@pytest.mark.parametrize("name", list(NESTING))
def test_nesting(world, name):
    plan, tables, layout = run_check(world, NESTING[name], key=name, what=name)
    run_check(world, NESTING[name], sort=world["sort"], key=name, what=name + " sorted")
    if name == "filter_children":  # year over 0001 .. 9999 under a filter: the global home, and the value kernel's
        from searchlite_amd import _native as N
        assert table_bytes(layout) > N.AGG_LDS_BYTES
    if name == "two_root_filters":
        q = 6
        for i, flt in ((0, "odd"), (1, "tree")):
            assert int(tables[i][q, 0, 0]) == sum(1 for s, d in world["docs"][q] if world["masks"][flt][s][d]) > 0


# ---- 8, 9: filter sources under a per-query filter; score order, sorted and scan batches ------------------------------
FILTERED = {"b": {"type": "filter", "filter": {"name": "odd"}, "aggs": {"h": dict(BOUNDED)}},
            "t": {"type": "filter", "filter": {"name": "tree"}, "aggs": {"s": {"type": "stats", "field": "x"}}},
            "h": dict(BOUNDED, aggs={"f": {"type": "filter", "filter": {"name": "tree"}}})}


def test_filter_sources_under_a_query_filter(world, oracle):
    """a bitmap filter and a filter tree as aggregation filters, while every other query has ANOTHER filter as its
    own: a doc that the query's filter rejects is counted nowhere"""
    W = world
    nq = len(W["offs"]) - 1
    qf = np.where(np.arange(nq) % 2 == 0, W["filter_ids"]["half"], -1).astype(np.int32)
    for f in ("odd", "tree"):
        got = W["ix"].fetch_filter(W["filter_ids"][f])
        for s, seg in enumerate(W["segs"]):
            alive = ~np.unpackbits(seg.deleted, bitorder="little")[:seg.n_docs].astype(bool) if seg.deleted is not None \
                else np.ones(seg.n_docs, bool)
            assert np.array_equal(got[s], W["masks"][f][s] & alive), f"filter {f} of segment {s}"
    want = oracle.search_batch_filtered(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], qf,
                                        {W["filter_ids"]["half"]: W["masks"]["half"]}, strategy=oracle.BM25)
    docs = docs_of(want)
    assert 0 < len(docs[6]) < len(W["docs"][6]) and len(docs[5]) == len(W["docs"][5])
    plan, tables, layout = run_check(W, FILTERED, docs=docs, key="filtered", what="filtered", q_filter=qf)
    run_check(W, FILTERED, docs=docs, sort=W["sort"], key="filtered", what="filtered sorted", q_filter=qf)
    half, odd = W["masks"]["half"], W["masks"]["odd"]
    assert int(tables[0][6, 0, 0]) == sum(1 for s, d in W["docs"][6] if half[s][d] and odd[s][d])


def test_scan_batch(world):
    """a match_all scan batch: every live doc (that the root filter passes) is aggregated"""
    W = world
    plan = planned(FILTERED, W["fields"])
    live = [(s, d) for s, seg in enumerate(W["segs"]) for d in range(seg.n_docs)
            if seg.deleted is None or not (seg.deleted[d >> 3] >> (d & 7)) & 1]
    third = W["masks"]["third"]
    docs = [live, [(s, d) for s, d in live if third[s][d]]]
    queries = [{"match_all": {}}, {"match_all": {}}]
    qf = np.array([-1, W["filter_ids"]["third"]], np.int32)
    want = expected(W, FILTERED, plan, docs, "scan")
    got = W["ix"].search_scan(queries, 11, aggs=plan, q_filter=qf)
    base = W["ix"].search_scan(queries, 11, q_filter=qf)
    for a, b_ in zip(got[:5], base[:5]):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b_).view(np.uint32)), "rows of the plain scan batch"
    assert got[4].tolist() == [len(d) for d in docs]
    check(plan, got[5], got[6], want, "scan")
    got = W["ix"].search_scan(queries, 0, sort=[W["sort"][0]], aggs=plan, q_filter=qf)
    check(plan, got[5], got[6], want, "sorted scan, k = 0")


# ---- 11: deleted docs ---------------------------------------------------------------------------------------------
def test_deleted_docs_are_counted_nowhere(oracle):
    import searchlite_amd as sa
    W = make_world(np.random.default_rng(11))
    W["segs"] = [copy.copy(s) for s in W["segs"]]
    with sa.GpuIndex([copy.copy(s) for s in W["segs"]]) as ix:
        W["ix"] = ix
        W["fields"], W["filter_ids"] = register(ix, W)
        search = lambda segs: docs_of(oracle.search_batch(segs, W["offs"], W["terms"], W["w"], W["k_all"], strategy=oracle.BM25))
        W["docs"] = search(W["segs"])
        before = run_check(W, FILTERED, what="before")[1]
        dead = np.random.default_rng(12).random(210) < 0.4
        ix.update_deleted(0, np.packbits(dead, bitorder="little"), 210 - int(dead.sum()))
        W["segs"][0].deleted, W["segs"][0].docs = np.packbits(dead, bitorder="little"), float(210 - int(dead.sum()))
        W["docs"] = search(W["segs"])
        assert not any(s == 0 and dead[d] for q in W["docs"] for s, d in q)
        after = run_check(W, FILTERED, what="after update_deleted")[1]
        assert int(after[0][6].sum()) < int(before[0][6].sum())


# ---- 12: refusals that need the index ------------------------------------------------------------------------------
def test_refusals(world):
    from searchlite_amd import _native as N, aggs as A
    W, ix = world, world["ix"]

    def fails(code, request, fields=None, word=None):
        with pytest.raises(N.SlgError) as ei:
            ix.search_aggs(W["offs"], W["terms"], W["w"], 11, planned(request, fields or W["fields"]))
        assert ei.value.code == code, ei.value
        assert word is None or word in str(ei.value), ei.value

    dh = lambda **kw: {"h": dict({"type": "date_histogram", "field": "ts"}, **kw)}
    fails(N.ERR_UNSUPPORTED, dh(calendar_interval="day"), word="SLG_MAX_AGG_CELLS")       # 3.65 M days
    fails(N.ERR_UNSUPPORTED, dh(calendar_interval="month"), word="SLG_MAX_AGG_CELLS")     # 119 988 months
    fails(N.ERR_UNSUPPORTED, dh(fixed_interval="1d"), word="SLG_MAX_AGG_CELLS")
    fails(N.ERR_UNSUPPORTED, {"t": {"type": "terms", "field": "kw", "aggs": dh(calendar_interval="quarter")}},
          word="SLG_MAX_AGG_CELLS")                                                       # 5 x 39 996 cells
    # a calendar instant out of range: the offset moves 0001-01-01 before the supported range; `missing` beyond it
    fails(N.ERR_UNSUPPORTED, dh(calendar_interval="year", offset="1ms"), word="calendar instant")
    fails(N.ERR_UNSUPPORTED, dh(calendar_interval="year", missing=D.MAX_MS + 1), word="calendar instant")
    fails(N.ERR_UNSUPPORTED, dh(calendar_interval="year", missing=D.MIN_MS - 1), word="calendar instant")
    ok = dh(calendar_interval="year", missing=D.MAX_MS + 1, hard_bounds={"min": str(D.MIN_MS), "max": str(D.MAX_MS)})
    run_check(W, ok, key="clamped", what="a missing the hard bounds cut off")
    # a value beyond +-2^53: in the column (an i64 that is no f64; an f64 beyond it), in `missing`
    big = [[[(1 << 53) + 1] if d == 3 else [d] for d in range(s.n_docs)] for s in W["segs"]]
    fails(N.ERR_UNSUPPORTED, {"h": {"type": "date_histogram", "field": "big", "fixed_interval": "1w"}},
          {"big": {"id": ix.add_agg_field(big, np.int64)}}, word="2^53")
    bigf = [[[2.0 ** 54] if d == 3 else [float(d)] for d in range(s.n_docs)] for s in W["segs"]]
    fails(N.ERR_UNSUPPORTED, {"h": {"type": "date_histogram", "field": "big", "fixed_interval": "1w"}},
          {"big": {"id": ix.add_agg_field(bigf, np.float64)}}, word="2^53")
    fails(N.ERR_UNSUPPORTED, dh(fixed_interval="1w", missing=2.0 ** 53 + 2), word="missing")
    # a date node on a keyword column
    fails(N.ERR_INVALID, {"h": {"type": "date_histogram", "field": "kw", "fixed_interval": "1s"}}, word="keyword")
    # an unknown filter id, a removed filter id
    flt = {"f": {"type": "filter", "filter": {"name": "x"}, "aggs": {"s": {"type": "stats", "field": "x"}}}}
    fails(N.ERR_INVALID, flt, dict(W["fields"], **{A.FILTERS: lambda body: 12345}), word="unknown filter id")
    gone = ix.add_filter(W["masks"]["odd"])
    mapped = dict(W["fields"], **{A.FILTERS: lambda body: gone})
    plan = planned(flt, mapped)
    *_, tables, layout = ix.search_aggs(W["offs"], W["terms"], W["w"], 11, plan)
    assert int(tables[0][6, 0, 0]) > 0
    with ix.prepare(W["offs"], W["terms"], W["w"], 11, aggs=plan) as kept:  # a prepared batch keeps its index state
        ix.remove_filter(gone)
        fails(N.ERR_INVALID, flt, mapped, word="unknown filter id")
        kept.run()
        assert np.array_equal(kept.aggs()[0], tables[0])
    # a scan batch hands its spec to the same checks
    with pytest.raises(N.SlgError) as ei:
        ix.search_scan([{"match_all": {}}], 11, aggs=planned(flt, mapped))
    assert ei.value.code == N.ERR_INVALID
    with pytest.raises(N.SlgError) as ei:
        ix.search_scan([{"match_all": {}}], 11, aggs=planned(dh(calendar_interval="day"), W["fields"]))
    assert ei.value.code == N.ERR_UNSUPPORTED


# ---- 13: the host mappings over the world -------------------------------------------------------------------------
def test_date_range_and_value_count(world):
    req = {"r": {"type": "date_range", "field": "ts", "keyed": True, "missing": "2024-01-01T00:00:00Z",
                 "ranges": [{"key": "before", "to": "1969-12-31T23:59:59.999Z"},
                            {"from": "1970-01-01T00:00:00Z", "to": "2023-12-31T23:59:59.999Z"},
                            {"key": "leap day", "from": "2024-02-29T00:00:00Z", "to": "2024-02-29T23:59:59.999Z"},
                            {"from": "1709164800000"}],
                 "aggs": {"n": {"type": "value_count", "field": "x", "missing": 0},
                          "h": {"type": "date_histogram", "field": "near", "calendar_interval": "week"}}},
           "n": {"type": "value_count", "field": "ts"}}
    plan, tables, layout = run_check(world, req, key="mappings", what="date_range, value_count")
    run_check(world, req, sort=world["sort"], key="mappings", what="date_range, value_count sorted")
    ts = world["cols"]["ts"]
    assert int(tables[0][6, 0, 0]["count"]) == sum(len(ts[s][d]) for s, d in world["docs"][6])
