"""The composite aggregation on the device (slg_batch_prepare_composite / _set_composite_after / _fetch_composite).

Expected: the oracle run with k >= the number of docs gives every matched doc; tests/composite_ref.py —
CompositeCollector and finalize_composite restated, checked against hand-derived answers in
tests/test_composite_ref.py — collects and finalizes them, the children of a bucket through tests/agg_date_ref.py.
Bar: tolerance 0 — keys (a float part by its bits), n_buckets, has_more, counts and children equal (the children's
sums too: every summed column here holds multiples of 0.25 of small magnitude, so any order of addition is exact),
zeros past n_buckets; the batch's rows, matched counts and aggregation tables bit-identical to the same batch without
the composite.

The world: three segments of 1300 / 900 / 700 docs (the second with tombstones), six queries: 0 the three most
frequent terms (nearly every live doc), 1 .. 3 three random terms, 4 no term, 5 one crafted list of 70 docs.
Columns: tag (6 keys in a dictionary order that is not byte order, non-ASCII among them: none, one, the same twice, or
two), pair (4 keys, two different on every doc), big (3000 keys, one or two), one (a single key on every doc), x (f64
multiples of 0.25 in [-6, 6], 0 .. 2 values), z (f64 around zero with -0.0, 0 .. 2 values), up / down (f64, one value
rising / falling with (segment, doc): keys arrive in ascending / descending order), u3 (f64, three values per doc, all
distinct over the world), ts (i64 milliseconds), n64 (i64), nf (f64 with an infinity), masks half and third.
The selection's edges come from the kernel's capacities (searchlite_amd._native.composite_cap, 3/4 of it the fill
limit): a wave's set is compacted whenever it passes the limit, which the worlds guarantee by pigeonhole over the
workgroup's four waves.
"""
import math

import numpy as np
import pytest

from tests import collapse_world as CW
from tests import composite_ref as R
from tests.util import _append_lists, random_queries, random_segment

pytestmark = pytest.mark.gpu

NO_TERM = 0xFFFFFFFF
SIZES = (1300, 900, 700)
VOCAB = 40
NQ = 6
TAG_KEYS = ["k3", "é", "a", "ab", "Z", "中"]
PAIR_KEYS = ["p2", "p0", "p3", "p1"]
BIG = 3000
BIG_KEYS = None  # (filled by build: w0000 .. w2999 in a shuffled dictionary order)
DAY = 86_400_000
F64 = {"x", "z", "up", "down", "u3", "nf", "lo31", "hi31"}
WAVES = 4


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return sa


def hits_of(all_hits):
    doc, seg, _, count = all_hits
    return [[(int(seg[q, i]), int(doc[q, i])) for i in range(int(count[q]))] for q in range(len(count))]


def build(oracle):
    global BIG_KEYS
    rng = np.random.default_rng(20261022)
    segs = [random_segment(rng, n, VOCAB, 25, k1=0.9, b=0.4) for n in SIZES]
    segs[0] = _append_lists(segs[0], [(np.sort(rng.choice(SIZES[0], size=70, replace=False)), np.ones(70))])
    segs[1] = CW.tombstoned(segs[1], rng, 0.15)
    offs, terms, w = random_queries(rng, NQ, 3, VOCAB, n_segs=3, weights=True)
    terms[0:3, :] = np.array([0, 1, 2], np.uint32)[:, None]
    for q in (4, 5):
        terms[3 * q:3 * q + 3, :] = NO_TERM
    terms[3 * 5, 0] = 40
    n_docs = [s.n_docs for s in segs]
    all_hits = oracle.search_batch(segs, offs, terms, w, sum(n_docs), strategy=oracle.BM25)
    BIG_KEYS = [f"w{int(i):04d}" for i in rng.permutation(BIG)]

    def tag():
        r = rng.random()
        a, b = (TAG_KEYS[int(j)] for j in rng.integers(0, len(TAG_KEYS), 2))
        return [] if r < 0.1 else [a] if r < 0.7 else [a, a] if r < 0.8 or a == b else [a, b]
    per_doc = lambda f: [[f(s, d) for d in range(n)] for s, n in enumerate(n_docs)]
    zpool = [-0.0, 0.0, 0.1, -0.1, 0.3, -0.3, 0.6, -0.6, 1e-320, -1e-320]
    cols = {
        "tag": per_doc(lambda s, d: tag()),
        "pair": per_doc(lambda s, d: [PAIR_KEYS[int(j)] for j in rng.choice(4, size=2, replace=False)]),
        "big": per_doc(lambda s, d: [BIG_KEYS[int(j)] for j in rng.integers(0, BIG, int(rng.integers(1, 3)))]),
        "one": per_doc(lambda s, d: ["only"]),
        "x": per_doc(lambda s, d: [float(v) / 4.0 for v in rng.integers(-24, 25, int(rng.integers(0, 3)))]),
        "z": per_doc(lambda s, d: [zpool[int(j)] for j in rng.integers(0, len(zpool), int(rng.integers(0, 3)))]),
        "up": per_doc(lambda s, d: [float(s * 100000 + d)]),
        "down": per_doc(lambda s, d: [float(1000000 - (s * 100000 + d))]),
        "u3": per_doc(lambda s, d: [float((s * 100000 + d) * 3 + j) for j in range(3)]),
        "ts": per_doc(lambda s, d: [int(rng.integers(0, 9)) * DAY + int(rng.integers(0, DAY)) for _ in range(int(rng.integers(0, 3)))]),
        "n64": per_doc(lambda s, d: [int(rng.integers(0, 50))]),
        "nf": per_doc(lambda s, d: [math.inf if (s, d) == (1, 5) else 1.0]),
    }
    masks = {"half": [rng.random(n) < 0.5 for n in n_docs], "third": [rng.random(n) < 0.33 for n in n_docs]}
    return dict(segs=segs, offs=offs, terms=terms, w=w, n_docs=n_docs, k_all=sum(n_docs), hits=hits_of(all_hits),
                cols=cols, masks=masks, keys_of={"tag": TAG_KEYS, "pair": PAIR_KEYS, "big": BIG_KEYS, "one": ["only"]})


def open_world(gpu, w):
    from searchlite_amd import aggs as A
    ix = w["ix"] = gpu.GpuIndex(w["segs"])
    fields = {}
    for name, keys in w["keys_of"].items():
        ord_of = {k: i for i, k in enumerate(keys)}
        ords = [[np.array([ord_of[v] for v in d], np.uint32) for d in seg] for seg in w["cols"][name]]
        fields[name] = {"id": ix.add_agg_keyword_field(ords, len(keys)), "keys": keys}
    for name, col in w["cols"].items():
        if name not in w["keys_of"]:
            fields[name] = {"id": ix.add_agg_field(col, np.float64 if name in F64 else np.int64)}
    w["filter_ids"] = {n: ix.add_filter(m) for n, m in w["masks"].items()}
    fields[A.FILTERS] = lambda body: w["filter_ids"][body["name"]]
    w["sort_ids"] = {"n64": ix.add_sort_field(w["cols"]["n64"], np.int64)}
    w["agg_fields"] = fields
    w["collected"] = {}
    return w


@pytest.fixture(scope="module")
def W(gpu, oracle):
    w = open_world(gpu, build(oracle))
    yield w
    w["ix"].close()


def T(name, field=None):
    return {"type": "terms", "name": name, "field": field or name}


def H(name, interval, field=None):
    return {"type": "histogram", "name": name, "field": field or name, "interval": interval}


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def collected(W, sources, hits, key):
    """composite_ref.collect per query, once per (sources, matched set)"""
    ck = (repr(sources), key)
    if ck not in W["collected"]:
        W["collected"][ck] = [R.collect(sources, W["cols"], F64, h) for h in hits]
    return W["collected"][ck]


def want_page(W, body, buckets, after):
    """composite_ref.respond from the collected buckets of one query"""
    from tests import agg_date_ref as D
    rows, has_more = R.finalize(body["sources"], buckets, body["size"], after)
    kids = body.get("aggs") or {}
    out = []
    for key, docs in rows:
        b = {"key": {s["name"]: p for s, p in zip(body["sources"], key)}, "doc_count": len(docs)}
        if kids:
            b["aggregations"] = D.respond(kids, D.run(kids, W["cols"], W["masks"], docs))
        out.append(b)
    resp = {"type": "composite", "buckets": out}
    if has_more and out:
        resp["after_key"] = out[-1]["key"]
    return resp


def assert_same_response(got, want, what):
    assert got["type"] == want["type"] == "composite"
    assert len(got["buckets"]) == len(want["buckets"]), f"{what}: {len(got['buckets'])} buckets, want {len(want['buckets'])}"
    for i, (g, w_) in enumerate(zip(got["buckets"], want["buckets"])):
        assert R.same_key(g["key"], w_["key"]), f"{what}: bucket {i} key {g['key']} want {w_['key']}"
        assert g["doc_count"] == w_["doc_count"], f"{what}: bucket {i} {g['key']} count"
        assert g.get("aggregations") == w_.get("aggregations"), f"{what}: bucket {i} {g['key']} children"
    assert ("after_key" in got) == ("after_key" in want), f"{what}: has_more"
    if "after_key" in want:
        assert R.same_key(got["after_key"], want["after_key"]), what


def check_raw(page, lay, what):
    """ascending keys below 1 << key_bits, zeros past n_buckets"""
    for q in range(len(page["n_buckets"])):
        n = int(page["n_buckets"][q])
        keys = [int(v) for v in page["keys"][q]]
        assert all(a < b for a, b in zip(keys[:n], keys[1:n])), f"{what}: query {q} keys not ascending"
        assert all(v < (1 << lay["key_bits"]) for v in keys[:n])
        assert not any(keys[n:]) and not page["counts"][q, n:].any(), f"{what}: query {q} rows past n_buckets"
        assert n == 0 or page["counts"][q, :n].min() >= 1
        for tab in page["children"]:
            assert not tab[q, n:].view(np.uint8).any(), f"{what}: query {q} child rows past n_buckets"
        assert int(page["has_more"][q]) in (0, 1)


def run_case(W, body, other=None, sort=None, k=7, q_filter=None, hits=None, key="world", what="", afters=None):
    """one composite batch against the reference and against the same batch without the composite.  afters: per query
    the `after` object (None: body's own for every query) -> (plan, layout, page, responses per query)"""
    from searchlite_amd import aggs as A
    what = f"{what} sources={[s['name'] for s in body['sources']]} size={body['size']} sort={sort} k={k}"
    ix = W["ix"]
    request = dict(other or {}, cmp=body)
    plan = A.agg_spec(request, W["agg_fields"])
    hits = W["hits"] if hits is None else hits
    afters = [body.get("after")] * NQ if afters is None else afters
    q = (W["offs"], W["terms"], W["w"])
    kw = dict(sort=None if sort is None else [(W["sort_ids"][f], o) for f, o in sort], q_filter=q_filter)
    has_aggs = plan.spec.n_nodes > 0
    with ix.prepare(*q, k, aggs=plan, **kw) as b:
        lay = b.composite_layout()
        if any(a is not None for a in afters):
            b.set_composite_after([A.composite_lower_bound(lay, plan, a) for a in afters])
        b.run()
        rows, matched, page = b.fetch(), b.matched_counts(), b.composite()
        tables = b.aggs() if has_aggs else []
    # the invariant: rows, matched counts and every table as without the composite
    if has_aggs:
        *base, base_matched, base_tables, _ = ix.search_aggs(*q, k, plan.spec, **kw)
        same(matched, base_matched, what + ": matched vs the aggregation batch")
        assert len(tables) == len(base_tables)
        for i, (a, b_) in enumerate(zip(tables, base_tables)):
            same(a, b_, f"{what}: table {i} vs the aggregation batch")
    elif sort is not None:
        *base, base_matched = ix.search_sorted(*q, k, kw["sort"], q_filter=q_filter)
        same(matched, base_matched, what + ": matched vs the sorted batch")
    else:
        with ix.prepare(*q, k, q_filter=q_filter) as plain:
            plain.run()
            base = plain.fetch()
    for a, b_, name in zip(rows, base, ("doc", "seg", "score", "count")):
        same(a, b_, f"{what}: rows differ in {name} from the batch without the composite")
    assert matched.tolist() == [len(h) for h in hits], what + ": matched"
    check_raw(page, lay, what)
    buckets = collected(W, body["sources"], hits, key)
    out = []
    for qi in range(NQ):
        got = A.shape_composite(plan, lay, page, qi)
        assert_same_response(got, want_page(W, body, buckets[qi], afters[qi]), f"{what}: query {qi}")
        out.append(got)
    return plan, lay, page, out


def cmp(sources, size, **kw):
    return dict({"type": "composite", "sources": sources, "size": size}, **kw)


# ---- 1. sources ---------------------------------------------------------------------------------------------------
def test_one_terms_source(W):
    _, lay, page, out = run_case(W, cmp([T("tag")], 4), what="terms")
    assert lay["key_bits"] == 3 and lay["sources"][0]["slots"] == 6
    assert len(out[0]["buckets"]) == 4 and "after_key" in out[0] and out[4]["buckets"] == []  # query 4 matches nothing
    assert [b["key"]["tag"] for b in out[0]["buckets"]] == ["Z", "a", "ab", "k3"]


def test_one_histogram_source(W):
    _, lay, _, out = run_case(W, cmp([H("x", 1.5)], 20), what="histogram")
    s = lay["sources"][0]
    assert s["first_id"] == -4 and s["zero_slot"] == 4 and s["slots"] == 10  # ids -4 .. 4, and the slot of -0.0
    assert len(out[0]["buckets"]) == 9 and "after_key" not in out[0]


def test_two_and_four_source_mixes(W):
    run_case(W, cmp([T("tag"), H("x", 2.0)], 50), what="two")
    run_case(W, cmp([H("x", 2.0), T("tag")], 7), what="two, the other way round")
    _, lay, _, out = run_case(W, cmp([T("pair"), H("x", 3.0), T("tag"), H("z", 0.25)], 100), what="four")
    assert lay["n_sources"] == 4 and [s["shift"] for s in lay["sources"]] == sorted((s["shift"] for s in lay["sources"]), reverse=True)
    assert len(out[0]["buckets"]) == 100 and "after_key" in out[0]


def test_k_zero_sorted_and_beside_aggregations(W):
    run_case(W, cmp([T("tag"), H("x", 2.0)], 9), k=0, what="k = 0")
    run_case(W, cmp([T("tag")], 9), sort=[("n64", "asc")], what="sorted")
    other = {"by_tag": {"type": "terms", "field": "tag", "aggs": {"s": {"type": "stats", "field": "x"}}},
             "card": {"type": "cardinality", "field": "tag"}}
    run_case(W, cmp([T("tag"), H("x", 2.0)], 9, aggs={"s": {"type": "stats", "field": "x"}}), other=other,
             what="beside an aggregation spec")
    run_case(W, cmp([T("tag")], 3), other=other, sort=[("n64", "desc")], k=0, what="beside a spec, sorted, k = 0")


def test_doc_filter_and_tombstones(W, oracle):
    qf = np.full(NQ, -1, np.int32)
    qf[0] = qf[2] = W["filter_ids"]["third"]
    want = oracle.search_batch_filtered(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], qf,
                                        {W["filter_ids"]["third"]: W["masks"]["third"]}, strategy=oracle.BM25)
    hits = hits_of(want)
    assert 0 < len(hits[0]) < len(W["hits"][0]) and len(hits[1]) == len(W["hits"][1])
    dead = W["segs"][1].deleted
    assert dead is not None and not any((dead[d >> 3] >> (d & 7)) & 1 for s, d in W["hits"][0] if s == 1)
    run_case(W, cmp([T("tag"), H("x", 2.0)], 11), q_filter=qf, hits=hits, key="third", what="filtered")


# ---- 2. the selection's edges -----------------------------------------------------------------------------------------
def test_more_keys_than_a_set_holds(W):
    from searchlite_amd import _native as N
    limit = lambda size: N.composite_cap(size) * 3 // 4
    big = collected(W, [T("big")], W["hits"], "world")
    assert len(big[0]) > WAVES * limit(3)  # some wave passes its fill limit, again and again
    for size in (1, 3):
        _, _, page, out = run_case(W, cmp([T("big")], size), what="big")
        assert int(page["n_buckets"][0]) == size and int(page["has_more"][0]) == 1
    wide = [H("u3", 1.0), T("pair")]
    assert len(collected(W, wide, W["hits"], "world")[0]) > WAVES * limit(N.MAX_COMPOSITE_SIZE)
    _, _, page, _ = run_case(W, cmp(wide, N.MAX_COMPOSITE_SIZE), what="wide")
    assert int(page["n_buckets"][0]) == N.MAX_COMPOSITE_SIZE and int(page["has_more"][0]) == 1


def test_exactly_size_and_one_more(W):
    n = len(collected(W, [T("tag"), H("x", 2.0)], W["hits"], "world")[0])
    assert n > 8
    _, _, page, _ = run_case(W, cmp([T("tag"), H("x", 2.0)], n), what="exactly size")
    assert int(page["n_buckets"][0]) == n and int(page["has_more"][0]) == 0
    _, _, page, out = run_case(W, cmp([T("tag"), H("x", 2.0)], n - 1), what="size + 1")
    assert int(page["n_buckets"][0]) == n - 1 and int(page["has_more"][0]) == 1  # the last key is withheld


@pytest.mark.parametrize("field", ["down", "up"])
def test_arrival_order(W, field):
    from searchlite_amd import _native as N
    # one key per doc, falling / rising with (segment, doc): under `down` every key is below the threshold when it comes
    for size in (3, N.MAX_COMPOSITE_SIZE):
        _, _, page, _ = run_case(W, cmp([H(field, 1.0)], size), what=field)
        assert int(page["n_buckets"][0]) == size and int(page["has_more"][0]) == 1


def test_one_key_everywhere(W):
    _, _, page, out = run_case(W, cmp([T("one")], 5), what="one key")  # in every segment and slice: one bucket
    assert out[0]["buckets"] == [{"key": {"one": "only"}, "doc_count": len(W["hits"][0])}] and "after_key" not in out[0]
    _, _, page, out = run_case(W, cmp([T("one"), T("tag")], 1), what="one key and tag")
    assert int(page["has_more"][0]) == 1


# ---- 3. paging ---------------------------------------------------------------------------------------------------------
def test_paging_covers_the_bucket_set(W):
    from searchlite_amd import aggs as A
    sources = [T("tag"), H("x", 2.0)]
    body = cmp(sources, 5, aggs={"s": {"type": "stats", "field": "x"}})
    plan = A.agg_spec({"cmp": body}, W["agg_fields"])
    buckets = collected(W, sources, W["hits"], "world")
    pages = [[] for _ in range(NQ)]
    afters, live = [None] * NQ, [True] * NQ
    with W["ix"].prepare(W["offs"], W["terms"], W["w"], 3, aggs=plan) as b:
        lay = b.composite_layout()
        for _ in range(40):
            # (a finished query is parked above every key: its pages stay empty)
            b.set_composite_after([A.composite_lower_bound(lay, plan, a) if on else 1 << lay["key_bits"]
                                   for a, on in zip(afters, live)])
            b.run()
            page = b.composite()
            check_raw(page, lay, "paging")
            for q in range(NQ):
                got = A.shape_composite(plan, lay, page, q)
                if not live[q]:
                    assert got["buckets"] == [] and "after_key" not in got
                    continue
                assert_same_response(got, want_page(W, body, buckets[q], afters[q]), f"page of query {q} after {afters[q]}")
                pages[q] += got["buckets"]
                live[q] = "after_key" in got
                afters[q] = got.get("after_key")
            if not any(live):
                break
        assert not any(live)
    for q in range(NQ):  # the concatenation is the full ascending list: no gap, no repeat
        full = want_page(W, dict(body, size=10 ** 6), buckets[q], None)
        assert_same_response({"type": "composite", "buckets": pages[q]}, full, f"all pages of query {q}")
    assert len(pages[0]) > 10


def test_after_values(W):
    sources = [T("tag"), H("x", 2.0)]
    rows, _ = R.finalize(sources, collected(W, sources, W["hits"], "world")[0], 10 ** 6)
    keys = [{"tag": k[0], "x": k[1]} for k, _ in rows]
    cases = {"an existing key": keys[3], "between keys": {"tag": keys[3]["tag"], "x": keys[3]["x"] + 0.5},
             "an absent string": {"tag": "aa", "x": 0.0}, "below all": {"tag": "", "x": -1e9},
             "the last key": keys[-1], "above all": {"tag": "\U0010ffff", "x": 0.0},
             "above all in the last part": {"tag": keys[-1]["tag"], "x": 1e9},
             "ignored: a name is missing": {"tag": "a"}, "ignored: a wrong type": {"tag": "a", "x": "0"}}
    for name, after in cases.items():
        _, _, page, out = run_case(W, cmp(sources, 4, after=after), what="after = " + name)
        if name in ("the last key", "above all", "above all in the last part"):
            assert out[0]["buckets"] == [] and int(page["has_more"][0]) == 0
        if name.startswith("ignored") or name == "below all":
            assert R.same_key(out[0]["buckets"][0]["key"], keys[0])
        if name == "an existing key":
            assert R.same_key(out[0]["buckets"][0]["key"], keys[4])


# ---- 4. -0.0 -----------------------------------------------------------------------------------------------------------
def test_two_zero_buckets(W):
    _, lay, _, out = run_case(W, cmp([H("z", 0.25)], 20), what="zeros")
    xs = [b["key"]["z"] for b in out[0]["buckets"]]
    at = [i for i, v in enumerate(xs) if v == 0.0]
    assert len(at) == 2 and at[1] == at[0] + 1
    assert math.copysign(1.0, xs[at[0]]) == -1.0 and math.copysign(1.0, xs[at[1]]) == 1.0
    assert lay["sources"][0]["zero_slot"] == -lay["sources"][0]["first_id"] >= 0
    _, _, _, out = run_case(W, cmp([H("z", 0.25)], 1, after={"z": -0.0}), what="after -0.0")
    assert R.f64_order(out[0]["buckets"][0]["key"]["z"]) == R.f64_order(0.0)
    _, _, _, out = run_case(W, cmp([H("z", 0.25)], 1, after={"z": 0.0}), what="after 0.0")
    assert out[0]["buckets"][0]["key"]["z"] == 0.25
    run_case(W, cmp([T("tag"), H("z", 0.25)], 30, after={"tag": "a", "z": -0.0}), what="after (a, -0.0)")


# ---- 5. key width, ord_rank ------------------------------------------------------------------------------------------------
def test_key_width(gpu, oracle):
    from searchlite_amd import _native as N, aggs as A
    rng = np.random.default_rng(7)
    seg = random_segment(rng, 8, 3, 4, k1=0.9, b=0.4)
    seg = _append_lists(seg, [([0, 1], [1, 1])])  # (term 3: the two docs with values)
    ix = gpu.GpuIndex([seg])
    try:
        rest = [[] for _ in range(6)]
        cols = {"lo31": [[[-1.0e9], [1.0e9]] + rest], "hi31": [[[1.0e9, -1.0e9], [1.0e9]] + rest],
                "t2": [[["a"], ["b", "a"]] + rest], "t3": [[["a"], ["c"]] + rest]}
        keys_of = {"t2": ["b", "a"], "t3": ["a", "b", "c"]}
        fields = {}
        for name, col in cols.items():
            if name in keys_of:
                ord_of = {k: i for i, k in enumerate(keys_of[name])}
                fields[name] = {"id": ix.add_agg_keyword_field([[np.array([ord_of[v] for v in d], np.uint32) for d in s]
                                                                for s in col], len(keys_of[name])), "keys": keys_of[name]}
            else:
                fields[name] = {"id": ix.add_agg_field(col, np.float64)}
        offs, terms, w = np.array([0, 1], np.uint32), np.array([[3]], np.uint32), np.ones(1, np.float32)
        sources = [H("lo31", 1.0), T("t2"), H("hi31", 1.0)]
        body = cmp(sources, 10)
        plan = A.agg_spec({"cmp": body}, fields)
        with ix.prepare(offs, terms, w, 2, aggs=plan) as b:
            lay = b.composite_layout()
            assert [s["bits"] for s in lay["sources"]] == [31, 1, 31] and lay["key_bits"] == 63
            assert lay["sources"][0]["slots"] == 2 * 10 ** 9 + 2 and lay["sources"][0]["zero_slot"] == 10 ** 9
            b.run()
            assert b.matched_counts().tolist() == [2]
            page = b.composite()
            got = A.shape_composite(plan, lay, page, 0)
            want = R.respond(body, cols, F64, {}, [(0, 0), (0, 1)])
            assert_same_response(got, want, "63 bits")
            assert len(got["buckets"]) == 4 and int(page["keys"][0, 3]) >> 62 == 1
            # the page behind the second bucket, and behind the last
            for i, n_left in ((1, 2), (3, 0)):
                b.set_composite_after([A.composite_lower_bound(lay, plan, got["buckets"][i]["key"])])
                b.run()
                nxt = A.shape_composite(plan, lay, b.composite(), 0)
                assert_same_response(nxt, R.respond(dict(body, after=got["buckets"][i]["key"]), cols, F64, {},
                                                    [(0, 0), (0, 1)]), "63 bits, paged")
                assert len(nxt["buckets"]) == n_left
        with pytest.raises(N.SlgError) as ei:  # one more bit
            ix.prepare(offs, terms, w, 2, aggs=A.agg_spec({"cmp": cmp([H("lo31", 1.0), T("t3"), H("hi31", 1.0)], 10)}, fields))
        assert ei.value.code == N.ERR_UNSUPPORTED and "63 bits" in str(ei.value)
        with pytest.raises(N.SlgError) as ei:  # an id at 2^31
            ix.prepare(offs, terms, w, 2, aggs=A.agg_spec({"cmp": cmp([H("lo31", 0.25)], 10)}, fields))
        assert ei.value.code == N.ERR_UNSUPPORTED and "2^31" in str(ei.value)
    finally:
        ix.close()


def test_ord_rank_given_or_presorted(W):
    """a non-identity permutation over the world's dictionary, and NULL over a dictionary registered in key order,
    give the same buckets"""
    from searchlite_amd import aggs as A
    body = cmp([T("tag"), H("x", 2.0)], 12)
    plan, lay, page, out = run_case(W, body, what="ranked")
    assert plan.composite["sources"][0]["rank"].tolist() != list(range(len(TAG_KEYS)))
    ix = W["ix"]
    sorted_keys = sorted(TAG_KEYS, key=lambda s: s.encode("utf-8"))
    ord_of = {k: i for i, k in enumerate(sorted_keys)}
    fid = ix.add_agg_keyword_field([[np.array([ord_of[v] for v in d], np.uint32) for d in seg] for seg in W["cols"]["tag"]],
                                   len(sorted_keys))
    fields = dict(W["agg_fields"], tag={"id": fid, "keys": sorted_keys})
    plan2 = A.agg_spec({"cmp": body}, fields)
    assert plan2.composite["sources"][0]["rank"].tolist() == list(range(len(TAG_KEYS)))
    plan2.composite["spec"].sources[0].ord_rank = None
    with ix.prepare(W["offs"], W["terms"], W["w"], 7, aggs=plan2) as b:
        b.run()
        page2, lay2 = b.composite(), b.composite_layout()
    assert lay2 == lay
    for name in ("keys", "n_buckets", "has_more", "counts"):
        same(page2[name], page[name], "presorted: " + name)
    assert [A.shape_composite(plan2, lay2, page2, q) for q in range(NQ)] == out


# ---- 6. children ---------------------------------------------------------------------------------------------------------
KIDS = {"s": {"type": "stats", "field": "x"}, "t": {"type": "terms", "field": "tag"},
        "h": {"type": "histogram", "field": "x", "interval": 1.0}}
KIDS_EXT = dict(KIDS, f={"type": "filter", "filter": {"name": "half"}},
                d={"type": "date_histogram", "field": "ts", "fixed_interval": "1d"})


@pytest.mark.parametrize("kids", [KIDS, KIDS_EXT], ids=["plain", "ext"])
def test_children_in_lds(W, kids):
    from searchlite_amd import _native as N
    plan, lay, page, out = run_case(W, cmp([T("tag"), H("z", 0.5)], 12, aggs=kids), what="children, LDS")
    cells = sum(x["parent_rows"] * x["rows"] * (32 if x["is_stats"] else 4) for x in lay["children"]) + 4 * lay["size"]
    assert cells <= N.AGG_LDS_BYTES and all(x["parent_rows"] == 12 for x in lay["children"])
    assert out[0]["buckets"][0]["aggregations"]["s"]["count"] > 0


@pytest.mark.parametrize("kids", [KIDS, KIDS_EXT], ids=["plain", "ext"])
def test_children_in_device_memory(W, kids):
    from searchlite_amd import _native as N
    plan, lay, page, out = run_case(W, cmp([T("big"), T("tag")], 700, aggs=kids), what="children, global")
    cells = sum(x["parent_rows"] * x["rows"] * (32 if x["is_stats"] else 4) for x in lay["children"]) + 4 * lay["size"]
    assert cells > N.AGG_LDS_BYTES and len(out[0]["buckets"]) == 700


# ---- 7. rejections against the index -------------------------------------------------------------------------------------
def test_index_rejections(W):
    from searchlite_amd import _native as N, aggs as A, searcher
    ix, q = W["ix"], (W["offs"], W["terms"], W["w"])

    def refused(body, code, word, fields=None, patch=None):
        plan = A.agg_spec({"cmp": body}, fields or W["agg_fields"])
        if patch:
            patch(plan)
        with pytest.raises(N.SlgError) as ei:
            ix.prepare(*q, 5, aggs=plan)
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    refused(cmp([H("n64", 1.0)], 5), N.ERR_UNSUPPORTED, "i64")
    refused(cmp([H("nf", 1.0)], 5), N.ERR_UNSUPPORTED, "non-finite")
    refused(cmp([T("tag")], 5), N.ERR_INVALID, "unknown agg field", fields=dict(W["agg_fields"], tag={"id": 999, "keys": TAG_KEYS}))
    wrong = dict(W["agg_fields"], tag={"id": W["agg_fields"]["x"]["id"], "keys": TAG_KEYS})
    refused(cmp([T("tag")], 5), N.ERR_INVALID, "numeric field", fields=wrong)
    wrong = dict(W["agg_fields"], x={"id": W["agg_fields"]["tag"]["id"]})
    refused(cmp([H("x", 1.0)], 5), N.ERR_INVALID, "keyword field", fields=wrong)
    for bad in ([0, 1, 2, 3, 4, 4], [0, 1, 2, 3, 4, 6]):  # a repeat, a rank beyond the dictionary
        arr = np.array(bad, np.uint32)

        def patch(plan, arr=arr):
            plan.composite["spec"].sources[0].ord_rank = arr.ctypes.data
        refused(cmp([T("tag")], 5), N.ERR_INVALID, "permutation", patch=patch)
    # size x (1 + child cells) over the cell limit; the spec's own cells count
    refused(cmp([T("tag")], 1024, aggs={"b": {"type": "terms", "field": "big"}}), N.ERR_UNSUPPORTED, "SLG_MAX_AGG_CELLS")
    spec_alone = {"h": {"type": "histogram", "field": "up", "interval": 3.4}}  # 59030 rows: within the limit alone
    ix.prepare(*q, 5, aggs=A.agg_spec(spec_alone, W["agg_fields"])).close()
    plan = A.agg_spec(dict(spec_alone, cmp=cmp([T("tag")], 1024, aggs={"t": {"type": "terms", "field": "tag"}})),
                      W["agg_fields"])  # + 1024 x (1 + 6) cells
    with pytest.raises(N.SlgError) as ei:
        ix.prepare(*q, 5, aggs=plan)
    assert ei.value.code == N.ERR_UNSUPPORTED and "SLG_MAX_AGG_CELLS" in str(ei.value)
    # a composite batch does not run sharded
    b = ix.prepare(*q, 5, aggs=A.agg_spec({"cmp": cmp([T("tag")], 5)}, W["agg_fields"]))
    try:
        group = searcher.ShardGroup(ix, 0, 1, searcher.shard_unique_id(), len(W["segs"]))
        try:
            with pytest.raises(N.SlgError) as ei:
                b.run_sharded(group)
            assert ei.value.code == N.ERR_UNSUPPORTED
        finally:
            group.close()
    finally:
        b.close()
    # the composite calls on a batch of another kind
    with ix.prepare(*q, 5) as plain:
        plain.run()
        lib = plain._lib
        assert lib.slg_batch_composite_layout(plain._h, None) == N.ERR_INVALID
        assert lib.slg_batch_set_composite_after(plain._h, None) == N.ERR_INVALID
        assert lib.slg_batch_fetch_composite(plain._h, None, None, None) == N.ERR_INVALID
    # the other batch kinds take no composite
    with pytest.raises(N.SlgError) as ei:
        ix.prepare(*q, 5, aggs=A.agg_spec({"cmp": cmp([T("tag")], 5)}, W["agg_fields"]), cursors=[None] * NQ)
    assert ei.value.code == N.ERR_UNSUPPORTED


# ---- 8. a second run -------------------------------------------------------------------------------------------------------
def test_second_run_is_bit_identical(W):
    from searchlite_amd import aggs as A
    plan = A.agg_spec({"cmp": cmp([T("big"), H("x", 2.0)], 300, aggs={"s": {"type": "stats", "field": "x"}})},
                      W["agg_fields"])

    def snap(b):
        p = b.composite()
        return [p["keys"], p["n_buckets"], p["has_more"], p["counts"]] + p["children"]
    with W["ix"].prepare(W["offs"], W["terms"], W["w"], 7, aggs=plan) as b:
        lay = b.composite_layout()
        b.run()
        first = snap(b)
        b.run()
        for x, y in zip(snap(b), first):
            same(x, y, "second run")
        b.set_composite_after([A.composite_lower_bound(lay, plan, {"big": "w1500", "x": 0.0})] * NQ)
        b.run()
        moved = snap(b)
        assert not np.array_equal(moved[0], first[0])
        b.set_composite_after(None)
        b.run()
        for x, y in zip(snap(b), first):
            same(x, y, "after set_composite_after(NULL)")


def test_one_shot_form(W):
    """slg_search_batch_composite = prepare + run + fetch of the first page"""
    import ctypes as C
    from searchlite_amd import _native as N, aggs as A
    ix, k, nq, n_segs = W["ix"], 7, NQ, len(W["segs"])
    body = cmp([T("tag"), H("x", 2.0)], 9, aggs={"s": {"type": "stats", "field": "x"}})
    other = {"by_tag": {"type": "terms", "field": "tag"}}
    plan = A.agg_spec(dict(other, cmp=body), W["agg_fields"])
    with ix.prepare(W["offs"], W["terms"], W["w"], k, aggs=plan) as b:
        lay = b.composite_layout()
        b.run()
        rows, matched, page, tables = b.fetch(), b.matched_counts(), b.composite(), b.aggs()
    terms = np.ascontiguousarray(W["terms"], np.uint32)
    w = np.ascontiguousarray(W["w"], np.float32)
    queries = (N.Query * nq)()
    for q in range(nq):
        a, e = int(W["offs"][q]), int(W["offs"][q + 1])
        queries[q] = N.Query(e - a, terms.ctypes.data + a * n_segs * 4, w.ctypes.data + a * 4)
    cc, sc = len(TAG_KEYS) + 9, 9  # the spec's count cells and the composite's count row; the stats child's cells
    doc, seg = np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.uint32)
    score, count = np.zeros((nq, k), np.float32), np.zeros(nq, np.uint32)
    m, counts, stats = np.zeros(nq, np.uint64), np.zeros((nq, cc), np.uint64), np.zeros((nq, sc), A.STATS_DTYPE)
    keys, nb, more = np.zeros((nq, 9), np.uint64), np.zeros(nq, np.uint32), np.zeros(nq, np.uint32)
    p = lambda a: a.ctypes.data
    rc = ix._lib.slg_search_batch_composite(ix._h, C.addressof(queries), nq, None, None, None, C.addressof(plan.spec),
                                            C.addressof(plan.composite["spec"]), k, 1, p(doc), p(seg), p(score), p(count),
                                            p(m), p(counts), p(stats), p(keys), p(nb), p(more))
    assert rc == N.OK, ix._lib.slg_last_error()
    for a, b_, name in zip((doc, seg, score, count), rows, ("doc", "seg", "score", "count")):
        same(a, b_, "one shot: " + name)
    same(m, matched, "one shot: matched")
    same(keys, page["keys"], "one shot: keys")
    same(nb, page["n_buckets"], "one shot: n_buckets")
    same(more, page["has_more"], "one shot: has_more")
    assert lay["count_offset"] == len(TAG_KEYS)
    same(counts[:, :len(TAG_KEYS)], tables[0][:, 0, :], "one shot: the spec's table")
    same(counts[:, len(TAG_KEYS):], page["counts"], "one shot: the composite's counts")
    same(stats, page["children"][0][:, :, 0], "one shot: the stats child")
