"""significant_terms and rare_terms on the device (slg_batch_prepare_term_buckets / _fetch_term_buckets).

Expected: the oracle run with k >= the number of docs gives every matched doc; tests/term_buckets_ref.py — both
collectors, the merge and finalize restated, checked against hand-derived answers in tests/test_term_buckets_ref.py —
answers with per_segment=False (the device's all-segment counting, with the reference's per-segment-presence sum of
bg_count); the children of a bucket through tests/agg_date_ref.py.
Bar: tolerance 0 — keys, doc counts, background counts, the two totals, n_buckets, the BITS of every score and the
children equal (the children's sums too: every summed column here holds multiples of 0.25 of small magnitude, so any
order of addition is exact), zeros past n_buckets; the batch's rows, matched counts and aggregation tables bit-identical
to the same batch without the spec.

The world: three segments of 1300 / 900 / 700 docs (the second with tombstones), six queries: 0 the three most frequent
terms (nearly every live doc), 1 .. 3 three random terms, 4 no term, 5 one crafted list of 70 docs of segment 0 (it
matches nothing in segments 1 and 2: its keys are in ONE segment's foreground, most keys in the background only).
Columns: tag (6 keys in a dictionary order that is not byte order, non-ASCII among them: none, one, the same twice, or
two), tagw (tag's ordinals under a dictionary of 9000 keys: the global home of every kernel), big (3000 keys, one or
two: the LDS home of the count walk and of the background), uniq (six keys of its own on every doc, 17400 in all:
more qualifying rows than the per-wave sets of the select hold at any size), one (a single key on every doc), x (f64
multiples of 0.25, 0 .. 2 values), n64 (an i64 sort column), masks half, third, none (no doc) and tree (a filter tree:
tag in {a, Z}).
"""
import numpy as np
import pytest

from tests import collapse_world as CW
from tests import term_buckets_ref as R
from tests.util import _append_lists, random_queries, random_segment

pytestmark = pytest.mark.gpu

NO_TERM = 0xFFFFFFFF
SIZES = (1300, 900, 700)
VOCAB = 40
NQ = 6
TAG_KEYS = ["k3", "é", "a", "ab", "Z", "中"]
WIDE = 9000
BIG = 3000
PER_DOC = 6
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


def dead_set(seg):
    if seg.deleted is None:
        return None
    bits = np.unpackbits(np.asarray(seg.deleted, np.uint8), bitorder="little")[:seg.n_docs]
    return set(int(d) for d in np.nonzero(bits)[0])


def build(oracle):
    rng = np.random.default_rng(20261101)
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
    big_keys = [f"w{int(i):04d}" for i in rng.permutation(BIG)]
    n_uniq = PER_DOC * sum(n_docs)
    uniq_keys = [f"u{int(i):05d}" for i in rng.permutation(n_uniq)]
    base = np.cumsum([0] + n_docs)

    def tag():
        r = rng.random()
        a, b = (TAG_KEYS[int(j)] for j in rng.integers(0, len(TAG_KEYS), 2))
        return [] if r < 0.1 else [a] if r < 0.7 else [a, a] if r < 0.8 or a == b else [a, b]
    per_doc = lambda f: [[f(s, d) for d in range(n)] for s, n in enumerate(n_docs)]
    cols = {
        "tag": per_doc(lambda s, d: tag()),
        "big": per_doc(lambda s, d: [big_keys[int(j)] for j in rng.integers(0, BIG, int(rng.integers(1, 3)))]),
        "uniq": per_doc(lambda s, d: [uniq_keys[PER_DOC * (int(base[s]) + d) + j] for j in range(PER_DOC)]),
        "one": per_doc(lambda s, d: ["only"]),
        "x": per_doc(lambda s, d: [float(v) / 4.0 for v in rng.integers(-24, 25, int(rng.integers(0, 3)))]),
        "n64": per_doc(lambda s, d: [int(rng.integers(0, 50))]),
    }
    cols["tagw"] = cols["tag"]
    masks = {"half": [rng.random(n) < 0.5 for n in n_docs], "third": [rng.random(n) < 0.33 for n in n_docs],
             "none": [np.zeros(n, bool) for n in n_docs],
             "tree": [np.array([any(v in ("a", "Z") for v in d) for d in seg], bool) for seg in cols["tag"]]}
    keys_of = {"tag": TAG_KEYS, "tagw": TAG_KEYS + [f"~{i:04d}" for i in range(WIDE - len(TAG_KEYS))], "big": big_keys,
               "uniq": uniq_keys, "one": ["only"]}
    return dict(segs=segs, offs=offs, terms=terms, w=w, n_docs=n_docs, k_all=sum(n_docs), hits=hits_of(all_hits),
                cols=cols, masks=masks, keys_of=keys_of, deleted=[dead_set(s) for s in segs])


def register_keyword(ix, col, keys):
    ord_of = {k: i for i, k in enumerate(keys)}
    ords = [[np.array([ord_of[v] for v in d], np.uint32) for d in seg] for seg in col]
    return ix.add_agg_keyword_field(ords, len(keys))


def open_world(gpu, w):
    from searchlite_amd import aggs as A, filters as F
    ix = w["ix"] = gpu.GpuIndex(w["segs"])
    fields = {name: {"id": register_keyword(ix, w["cols"][name], keys), "keys": keys} for name, keys in w["keys_of"].items()}
    fields["x"] = {"id": ix.add_agg_field(w["cols"]["x"], np.float64)}
    w["filter_ids"] = {n: ix.add_filter(m) for n, m in w["masks"].items() if n != "tree"}
    tree = F.compile_filter({"KeywordIn": {"field": "tag", "values": ["a", "Z"]}},
                            {"tag": {"id": fields["tag"]["id"], "kind": "keyword", "keys": TAG_KEYS}})
    w["filter_ids"]["tree"] = ix.add_filter_trees([tree])[0]
    fields[A.FILTERS] = lambda body: w["filter_ids"][body["name"]]
    w["sort_ids"] = {"n64": ix.add_sort_field(w["cols"]["n64"], np.int64)}
    w["agg_fields"] = fields
    w["wanted"] = {}
    return w


@pytest.fixture(scope="module")
def W(gpu, oracle):
    w = open_world(gpu, build(oracle))
    yield w
    w["ix"].close()


def SIG(field, size, **kw):
    return dict({"type": "significant_terms", "field": field, "size": size}, **kw)


def RARE(field, size, **kw):
    return dict({"type": "rare_terms", "field": field, "size": size}, **kw)


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def wanted(W, body, hits, key, per_segment=False):
    """term_buckets_ref.respond per query, once per (body without children, matched set)"""
    bare = {k: v for k, v in body.items() if k != "aggs"}
    ck = (repr(sorted(bare.items(), key=repr)), key, per_segment)
    if ck not in W["wanted"]:
        W["wanted"][ck] = [R.respond(bare, W["cols"], W["n_docs"], W["deleted"], W["masks"], h, per_segment) for h in hits]
    return W["wanted"][ck]


def check_node(W, body, nd, lay, got, want, what):
    """one node of one batch against the reference's responses of every query: raw arrays, then the shaped children"""
    from searchlite_amd import aggs as A
    from tests import agg_date_ref as D
    sig = body["type"] == "significant_terms"
    keys = nd["keys"]
    kids = body.get("aggs") or {}
    for q in range(len(want)):   # (NQ here; tests/test_gpu_lifecycle.py brings its own queries)
        wq, n = want[q], int(got["n_buckets"][q])
        at = f"{what}: query {q}"
        assert n == len(wq["buckets"]), f"{at}: {n} buckets, want {len(wq['buckets'])}"
        assert [keys[int(o)] for o in got["ords"][q, :n]] == [b["key"] for b in wq["buckets"]], f"{at}: keys"
        assert got["doc_counts"][q, :n].tolist() == [b["doc_count"] for b in wq["buckets"]], f"{at}: doc counts"
        for name in ("ords", "doc_counts", "bg_counts", "score_bits"):  # rows past n_buckets are zero
            assert not got[name][q, n:].any(), f"{at}: {name} past n_buckets"
        if sig:
            assert got["bg_counts"][q, :n].tolist() == [b["bg_count"] for b in wq["buckets"]], f"{at}: bg counts"
            assert got["score_bits"][q, :n].tolist() == [R.score_bits(b["score"]) for b in wq["buckets"]], f"{at}: score bits"
            assert int(got["doc_count"][q]) == wq["doc_count"] and int(got["bg_count"][q]) == wq["bg_count"], f"{at}: totals"
        else:  # a rare node returns neither
            assert not got["bg_counts"][q].any() and not got["score_bits"][q].any(), f"{at}: a rare node's zero arrays"
            assert int(got["doc_count"][q]) == 0 and int(got["bg_count"][q]) == 0, f"{at}: a rare node's totals"
        if not kids:
            assert got["counts"] is None and got["children"] == []
            continue
        assert got["counts"][q, :n].tolist() == [b["doc_count"] for b in wq["buckets"]], f"{at}: the count cells"
        assert not got["counts"][q, n:].any()
        for tab in got["children"]:
            assert not tab[q, n:].view(np.uint8).any(), f"{at}: child rows past n_buckets"
        for r, b in enumerate(wq["buckets"]):
            have = A.shape(nd["children"], lay["children"], got["children"], q, prow=r)
            assert have == D.respond(kids, D.run(kids, W["cols"], W["masks"], b["docs"])), f"{at}: bucket {r} {b['key']} children"


def run_case(W, request, other=None, sort=None, k=7, q_filter=None, hits=None, key="world", what="", fields=None):
    """one batch with the term bucket nodes of `request` against the reference and against the same batch without them
    -> (plan, layout, fetched, wanted per node name)"""
    from searchlite_amd import aggs as A
    what = f"{what} {sorted(request)} sort={sort} k={k}"
    ix = W["ix"]
    plan = A.agg_spec(dict(other or {}, **request), fields or W["agg_fields"])
    hits = W["hits"] if hits is None else hits
    q = (W["offs"], W["terms"], W["w"])
    kw = dict(sort=None if sort is None else [(W["sort_ids"][f], o) for f, o in sort], q_filter=q_filter)
    has_aggs = plan.spec.n_nodes > 0
    with ix.prepare(*q, k, aggs=plan, **kw) as b:
        lay = b.term_buckets_layout()
        b.run()
        rows, matched, got = b.fetch(), b.matched_counts(), b.term_buckets()
        tables = b.aggs() if has_aggs else []
    # the invariant: rows, matched counts and every table as without the spec
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
        same(a, b_, f"{what}: rows differ in {name} from the batch without the spec")
    assert matched.tolist() == [len(h) for h in hits], what + ": matched"
    want = {}
    for nd, nlay, ngot in zip(plan.term_buckets["nodes"], lay["nodes"], got["nodes"]):
        body = request[nd["name"]]
        want[nd["name"]] = wanted(W, body, hits, key)
        check_node(W, body, nd, nlay, ngot, want[nd["name"]], f"{what}: {nd['name']}")
    return plan, lay, got, want


# ---- 1. the two kinds, the queries ------------------------------------------------------------------------------------
def test_significant_and_rare_on_a_small_dictionary(W):
    _, _, got, want = run_case(W, {"s": SIG("tag", 3), "r": RARE("tag", 3, max_doc_count=400)}, what="tag")
    s, r = want["s"], want["r"]
    assert len(s[0]["buckets"]) == 3 and s[4]["buckets"] == [] and s[4]["doc_count"] == 0  # query 4 matches nothing ...
    live = sum(n - len(d or ()) for n, d in zip(W["n_docs"], W["deleted"]))
    assert s[4]["bg_count"] == live == s[0]["bg_count"]  # ... and every segment still adds its bg_total
    assert any(len(w["buckets"]) for w in r)
    # query 5 collects in segment 0 only: a bucket's bg_count is segment 0's background count of its key, below the
    # key's count over all segments (what the per-segment-presence sum is about)
    assert all(seg == 0 for seg, _ in W["hits"][5]) and len(W["hits"][5]) == 70
    bg0, _ = R.background(W["cols"]["tag"][0], W["n_docs"][0], W["deleted"][0], None)
    everywhere = {}
    for sgi in range(3):
        for k_, c in R.background(W["cols"]["tag"][sgi], W["n_docs"][sgi], W["deleted"][sgi], None)[0].items():
            everywhere[k_] = everywhere.get(k_, 0) + c
    for b in s[5]["buckets"]:
        assert b["bg_count"] == bg0[b["key"]] < everywhere[b["key"]]


def test_k_zero_sorted_filtered_and_beside_aggregations(W, oracle):
    req = {"s": SIG("tag", 4, aggs={"st": {"type": "stats", "field": "x"}}), "r": RARE("big", 5)}
    run_case(W, req, k=0, what="k = 0")
    run_case(W, req, sort=[("n64", "asc")], what="sorted")
    other = {"by_tag": {"type": "terms", "field": "tag", "aggs": {"st": {"type": "stats", "field": "x"}}},
             "card": {"type": "cardinality", "field": "tag"}}
    run_case(W, req, other=other, what="beside an aggregation spec")
    run_case(W, req, other=other, sort=[("n64", "desc")], k=0, what="beside a spec, sorted, k = 0")
    qf = np.full(NQ, -1, np.int32)
    qf[0] = qf[2] = W["filter_ids"]["third"]
    want = oracle.search_batch_filtered(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], qf,
                                        {W["filter_ids"]["third"]: W["masks"]["third"]}, strategy=oracle.BM25)
    hits = hits_of(want)
    assert 0 < len(hits[0]) < len(W["hits"][0]) and len(hits[1]) == len(W["hits"][1])
    run_case(W, req, q_filter=qf, hits=hits, key="third", what="doc filter")  # (the background ignores the doc filter)


# ---- 2. the selection ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 3, 1024])
def test_more_qualifying_rows_than_a_set_holds(W, size):
    from searchlite_amd import _native as N
    assert size <= N.MAX_TERM_BUCKET_SIZE
    limit = N.term_bucket_cap(size) * 3 // 4  # a wave's set is compacted when it passes this
    # every key of uniq is on one doc: every collected key qualifies for both kinds with count 1, and the order is the
    # key order alone.  More than WAVES x limit qualifying rows: some wave passes its fill limit (pigeonhole)
    n_rows = PER_DOC * len(W["hits"][0])
    assert n_rows > WAVES * limit
    # (a node each: two nodes over uniq's 17400 ordinals are more cells than a query may have)
    _, _, got_s, want_s = run_case(W, {"s": SIG("uniq", size)}, what=f"uniq, size {size}")
    _, _, got_r, want_r = run_case(W, {"r": RARE("uniq", size)}, what=f"uniq, size {size}")
    assert int(got_s["nodes"][0]["n_buckets"][0]) == size == int(got_r["nodes"][0]["n_buckets"][0])
    assert all(b["doc_count"] == 1 for b in want_s["s"][0]["buckets"])
    # the same keys under both orders: the `size` first in key byte order (every score is the same too)
    assert [b["key"] for b in want_r["r"][0]["buckets"]] == [b["key"] for b in want_s["s"][0]["buckets"]] == \
        sorted(b["key"] for b in want_s["s"][0]["buckets"])


def test_exactly_size_and_one_more(W):
    n = len(wanted(W, SIG("tag", 1000), W["hits"], "world")[1]["buckets"])
    assert n >= 4
    _, _, got, _ = run_case(W, {"s": SIG("tag", n)}, what="exactly size")
    assert int(got["nodes"][0]["n_buckets"][1]) == n
    _, _, got, _ = run_case(W, {"s": SIG("tag", n - 1)}, what="size + 1 rows")
    assert int(got["nodes"][0]["n_buckets"][1]) == n - 1
    m = len(wanted(W, RARE("big", 1024, max_doc_count=1), W["hits"], "world")[5]["buckets"])
    assert 4 <= m <= 1024
    for size in (m, m - 1):
        _, _, got, _ = run_case(W, {"r": RARE("big", size, max_doc_count=1)}, what=f"rare, {m} rows, size {size}")
        assert int(got["nodes"][0]["n_buckets"][5]) == size


def test_ties_by_key_bytes_with_ord_rank_given_or_null(W):
    """a non-identity permutation over the world's dictionary (non-ASCII keys among it), and NULL over the same column
    registered in key byte order, give the same response"""
    from searchlite_amd import aggs as A
    req = {"s": SIG("tag", 6, min_doc_count=0), "r": RARE("tag", 6, max_doc_count=10 ** 6)}
    plan, lay, got, want = run_case(W, req, what="ranked")
    assert plan.term_buckets["nodes"][0]["rank"].tolist() != list(range(len(TAG_KEYS)))
    ix = W["ix"]
    sorted_keys = sorted(TAG_KEYS, key=lambda s: s.encode("utf-8"))
    assert sorted_keys != TAG_KEYS  # (the world's dictionary is not in byte order)
    fid = register_keyword(ix, W["cols"]["tag"], sorted_keys)
    fields = dict(W["agg_fields"], tag={"id": fid, "keys": sorted_keys})
    plan2, lay2, got2, _ = run_case(W, req, what="presorted", fields=fields)
    assert all(nd["rank"] is None for nd in plan2.term_buckets["nodes"])
    assert not plan2.term_buckets["spec"].nodes[0].ord_rank
    for q in range(NQ):
        assert A.shape_term_buckets(plan, lay, got, q) == A.shape_term_buckets(plan2, lay2, got2, q)


# ---- 3. the count bounds -------------------------------------------------------------------------------------------------
def test_min_doc_count_edges(W):
    counts = sorted({b["doc_count"] for b in wanted(W, SIG("tag", 100, min_doc_count=0), W["hits"], "world")[2]["buckets"]})
    assert len(counts) >= 2
    c = counts[1]  # a count some key has exactly, with a smaller one below it
    for mdc in (0, 1, c, c + 1):
        _, _, got, want = run_case(W, {"s": SIG("tag", 100, min_doc_count=mdc)}, what=f"min_doc_count {mdc}")
        have = {b["doc_count"] for b in want["s"][2]["buckets"]}
        assert (c in have) == (mdc <= c) and (counts[0] in have) == (mdc <= counts[0])
    a, b = (wanted(W, SIG("tag", 100, min_doc_count=m), W["hits"], "world") for m in (0, 1))
    assert [R.strip(x) for x in a] == [R.strip(x) for x in b]  # (a bucket exists once a doc was counted in it)


def test_max_doc_count_edges(W):
    _, _, _, want = run_case(W, {"r": RARE("big", 1024)}, what="max_doc_count 1, the default")
    assert len(want["r"][1]["buckets"]) == 1024 and all(b["doc_count"] == 1 for b in want["r"][1]["buckets"])
    # the 70 docs of query 5 over tag's six keys: a count some key has exactly, with smaller ones below it
    counts = sorted({b["doc_count"] for b in wanted(W, RARE("tag", None, max_doc_count=10 ** 6), W["hits"], "world")[5]["buckets"]})
    assert len(counts) >= 3 and counts[0] > 1
    c = counts[2]
    for mdc in (c, c - 1, 1):
        _, _, got, want = run_case(W, {"r": RARE("tag", 6, max_doc_count=mdc)}, what=f"max_doc_count {mdc}")
        have = {b["doc_count"] for b in want["r"][5]["buckets"]}
        assert (c in have) == (c <= mdc) and (counts[0] in have) == (counts[0] <= mdc) and all(x <= mdc for x in have)


# ---- 4. the background ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flt", [None, "half", "tree", "none"])
def test_background_filters(W, flt):
    body = SIG("tag", 6) if flt is None else SIG("tag", 6, background_filter={"name": flt})
    _, _, got, want = run_case(W, {"s": body}, what=f"background {flt}")
    s = want["s"]
    live = [n - len(d or ()) for n, d in zip(W["n_docs"], W["deleted"])]
    if flt is None:
        assert s[0]["bg_count"] == sum(live)
        # tombstoned docs are not counted: segment 1 has deleted docs that hold the first bucket's key
        key = s[0]["buckets"][0]["key"]
        assert any(key in W["cols"]["tag"][1][d] for d in W["deleted"][1])
        raw = sum(1 for seg in W["cols"]["tag"] for d in seg if key in d)
        assert s[0]["buckets"][0]["bg_count"] < raw
        # a value held twice counts once
        assert any(len(d) == 2 and d[0] == d[1] for d in W["cols"]["tag"][0])
    elif flt == "none":  # no doc left: bg_count 0 and every score 0.0, the order falls back to (count desc, key asc)
        assert all(w["bg_count"] == 0 for w in s)
        assert all(b["bg_count"] == 0 and b["score"] == 0.0 for w in s for b in w["buckets"])
        assert not got["nodes"][0]["score_bits"].any() and got["nodes"][0]["n_buckets"][0] == 6
    else:
        assert 0 < s[0]["bg_count"] < sum(live)
    if flt == "tree":  # the live docs that hold a or Z
        assert s[0]["bg_count"] == sum(1 for m, dead in zip(W["masks"]["tree"], W["deleted"])
                                       for d in np.nonzero(m)[0] if int(d) not in (dead or ()))


def test_a_key_in_the_background_only_has_no_bucket(W):
    _, _, got, want = run_case(W, {"s": SIG("big", 1024, min_doc_count=0)}, what="big, all buckets")
    fg5 = {v for _, d in W["hits"][5] for v in W["cols"]["big"][0][d]}
    assert {b["key"] for b in want["s"][5]["buckets"]} == fg5 and len(fg5) < BIG // 10
    assert int(got["nodes"][0]["n_buckets"][5]) == len(fg5)


# ---- 5. the tables --------------------------------------------------------------------------------------------------------
def test_one_ordinal(W):
    _, _, got, want = run_case(W, {"s": SIG("one", 5), "r": RARE("one", 5, max_doc_count=10 ** 6)}, what="n_ords 1")
    assert [b["key"] for b in want["s"][0]["buckets"]] == ["only"] and want["s"][0]["buckets"][0]["score"] == 1.0
    assert want["r"][0]["buckets"][0]["doc_count"] == len(W["hits"][0])


def test_both_table_homes_give_the_same_answer(W):
    from searchlite_amd import _native as N
    kids = {"st": {"type": "stats", "field": "x"}, "t": {"type": "terms", "field": "tag"}}
    small = {"s": SIG("tag", 6, background_filter={"name": "half"}, aggs=kids), "r": RARE("tag", 6, max_doc_count=500)}
    wide = {"s": SIG("tagw", 6, background_filter={"name": "half"}, aggs=kids), "r": RARE("tagw", 6, max_doc_count=500)}
    assert 2 * 4 * len(TAG_KEYS) <= N.AGG_LDS_BYTES < 4 * WIDE  # LDS in every kernel / global in every kernel
    _, _, a, wa = run_case(W, small, what="LDS homes")
    _, _, b, wb = run_case(W, wide, what="global homes")
    for x, y in zip(a["nodes"], b["nodes"]):
        for name in ("ords", "doc_counts", "bg_counts", "score_bits", "n_buckets", "doc_count", "bg_count"):
            same(x[name], y[name], "homes: " + name)
    # big beside tagw: the count walk's table is global (4 B x 12000 > LDS), big's background is in LDS (4 B x 3000)
    assert 4 * (BIG + WIDE) > N.AGG_LDS_BYTES >= 4 * BIG
    run_case(W, {"s": SIG("big", 20, background_filter={"name": "third"}), "w": SIG("tagw", 3)}, what="mixed homes")


def test_cell_cap(W):
    from searchlite_amd import _native as N, aggs as A
    ix, q = W["ix"], (W["offs"], W["terms"], W["w"])
    cap = N.MAX_AGG_CELLS // 2  # n_ords foreground cells and n_ords background-sum cells
    at_cap = TAG_KEYS + [f"~{i:05d}" for i in range(cap - len(TAG_KEYS))]
    fields = dict(W["agg_fields"], tagc={"id": register_keyword(ix, W["cols"]["tag"], at_cap), "keys": at_cap})
    W["cols"]["tagc"] = W["cols"]["tag"]
    run_case(W, {"s": SIG("tagc", 6)}, what="at the cell cap", fields=fields)
    over = at_cap + ["~over"]
    fields = dict(W["agg_fields"], tagc={"id": register_keyword(ix, W["cols"]["tag"], over), "keys": over})
    with pytest.raises(N.SlgError) as ei:
        ix.prepare(*q, 5, aggs=A.agg_spec({"s": SIG("tagc", 6)}, fields))
    assert ei.value.code == N.ERR_UNSUPPORTED and "SLG_MAX_AGG_CELLS" in str(ei.value)
    # the cells of the aggregation spec and of the children count too
    with pytest.raises(N.SlgError) as ei:
        ix.prepare(*q, 5, aggs=A.agg_spec({"s": SIG("tagw", 1024, aggs={"b": {"type": "terms", "field": "big"}})}, W["agg_fields"]))
    assert ei.value.code == N.ERR_UNSUPPORTED and "SLG_MAX_AGG_CELLS" in str(ei.value)


# ---- 6. nodes ---------------------------------------------------------------------------------------------------------------
def test_four_nodes_two_sharing_a_background(W):
    req = {"a": SIG("tag", 3, background_filter={"name": "half"}),
           "b": SIG("tag", 6, min_doc_count=2, background_filter={"name": "half"}),  # the same (field, filter) as a
           "c": RARE("big", 7, max_doc_count=2),
           "d": SIG("big", 9, aggs={"st": {"type": "stats", "field": "x"}})}
    _, lay, got, want = run_case(W, req, what="four nodes")
    assert [n["row_offset"] for n in lay["nodes"]] == [0, 3, 9, 16] and lay["rows"] == 25
    assert want["a"][0]["bg_count"] == want["b"][0]["bg_count"] != want["d"][0]["bg_count"]


# ---- 7. children -------------------------------------------------------------------------------------------------------------
KIDS = {"st": {"type": "stats", "field": "x"}, "t": {"type": "terms", "field": "tag"},
        "f": {"type": "filter", "filter": {"name": "half"}}}


def child_bytes(nlay):
    return sum(x["parent_rows"] * x["rows"] * (32 if x["is_stats"] else 4) for x in nlay["children"]) + 12 * nlay["size"]


def test_children_in_lds(W):
    from searchlite_amd import _native as N
    _, lay, got, want = run_case(W, {"s": SIG("tag", 5, aggs=KIDS), "r": RARE("big", 12, max_doc_count=3, aggs=KIDS)},
                                 what="children, LDS")
    assert all(child_bytes(n) <= N.AGG_LDS_BYTES for n in lay["nodes"])
    assert all(x["parent_rows"] == n["size"] for n in lay["nodes"] for x in n["children"])
    assert got["nodes"][1]["children"][1][0, 0, 0]["count"] >= 0 and len(want["s"][0]["buckets"]) == 5


def test_children_in_device_memory(W):
    from searchlite_amd import _native as N
    _, lay, got, want = run_case(W, {"s": SIG("big", 700, aggs=KIDS), "r": RARE("big", 700, max_doc_count=2, aggs=KIDS),
                                     "n": SIG("tag", 4)}, what="children, global")
    assert all(child_bytes(n) > N.AGG_LDS_BYTES for n in lay["nodes"] if n["children"])
    assert len(want["s"][0]["buckets"]) == 700 and got["nodes"][0]["counts"] is None  # (n: no children, no cells)


# ---- 8. a second run, the one-shot form, rejections ----------------------------------------------------------------------------
def test_second_run_is_bit_identical(W):
    from searchlite_amd import aggs as A
    plan = A.agg_spec({"s": SIG("big", 300, background_filter={"name": "half"}, aggs={"st": {"type": "stats", "field": "x"}}),
                       "r": RARE("tag", 4, max_doc_count=300), "u": SIG("uniq", 1024)}, W["agg_fields"])

    def snap(b):
        out = []
        for nd in b.term_buckets()["nodes"]:
            out += [nd[n] for n in ("ords", "doc_counts", "bg_counts", "score_bits", "n_buckets", "doc_count", "bg_count")]
            out += ([nd["counts"]] if nd["counts"] is not None else []) + nd["children"]
        return out
    with W["ix"].prepare(W["offs"], W["terms"], W["w"], 7, aggs=plan) as b:
        b.run()
        first = snap(b)
        b.run()
        for x, y in zip(snap(b), first):
            same(x, y, "second run")


def test_one_shot_form(W):
    """slg_search_batch_term_buckets = prepare + run + fetch"""
    import ctypes as C
    from searchlite_amd import _native as N, aggs as A
    ix, k, nq, n_segs = W["ix"], 7, NQ, len(W["segs"])
    plan = A.agg_spec({"by_tag": {"type": "terms", "field": "tag"},
                       "s": SIG("tag", 4, aggs={"st": {"type": "stats", "field": "x"}}), "r": RARE("big", 5)}, W["agg_fields"])
    with ix.prepare(W["offs"], W["terms"], W["w"], k, aggs=plan) as b:
        lay = b.term_buckets_layout()
        b.run()
        rows, matched, got, tables = b.fetch(), b.matched_counts(), b.term_buckets(), b.aggs()
    terms = np.ascontiguousarray(W["terms"], np.uint32)
    w = np.ascontiguousarray(W["w"], np.float32)
    queries = (N.Query * nq)()
    for q in range(nq):
        a, e = int(W["offs"][q]), int(W["offs"][q + 1])
        queries[q] = N.Query(e - a, terms.ctypes.data + a * n_segs * 4, w.ctypes.data + a * 4)
    assert lay["rows"] == 9 and [n["row_offset"] for n in lay["nodes"]] == [0, 5]  # (r, then s: name order)
    cc, sc = len(TAG_KEYS) + 4, 4  # the spec's count cells and s's count row; the stats child's cells
    doc, seg = np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.uint32)
    score, count = np.zeros((nq, k), np.float32), np.zeros(nq, np.uint32)
    m, counts, stats = np.zeros(nq, np.uint64), np.zeros((nq, cc), np.uint64), np.zeros((nq, sc), A.STATS_DTYPE)
    ords, nb = np.zeros((nq, 9), np.uint32), np.zeros((nq, 2), np.uint32)
    dc, bg, sb = (np.zeros((nq, 9), np.uint64) for _ in range(3))
    ndc, nbg = np.zeros((nq, 2), np.uint64), np.zeros((nq, 2), np.uint64)
    p = lambda a: a.ctypes.data
    rc = ix._lib.slg_search_batch_term_buckets(ix._h, C.addressof(queries), nq, None, None, None, C.addressof(plan.spec),
                                               C.addressof(plan.term_buckets["spec"]), k, 1, p(doc), p(seg), p(score),
                                               p(count), p(m), p(counts), p(stats), p(ords), p(dc), p(bg), p(sb), p(nb),
                                               p(ndc), p(nbg))
    assert rc == N.OK, ix._lib.slg_last_error()
    for a, b_, name in zip((doc, seg, score, count), rows, ("doc", "seg", "score", "count")):
        same(a, b_, "one shot: " + name)
    same(m, matched, "one shot: matched")
    for i, nd in enumerate(got["nodes"]):
        r0, r1 = lay["nodes"][i]["row_offset"], lay["nodes"][i]["row_offset"] + lay["nodes"][i]["size"]
        for arr, name in ((ords, "ords"), (dc, "doc_counts"), (bg, "bg_counts"), (sb, "score_bits")):
            same(arr[:, r0:r1], nd[name], "one shot: " + name)
        same(nb[:, i], nd["n_buckets"], "one shot: n_buckets")
        same(ndc[:, i], nd["doc_count"], "one shot: doc_count")
        same(nbg[:, i], nd["bg_count"], "one shot: bg_count")
    assert lay["nodes"][1]["count_offset"] == len(TAG_KEYS)
    same(counts[:, :len(TAG_KEYS)], tables[0][:, 0, :], "one shot: the spec's table")
    same(counts[:, len(TAG_KEYS):], got["nodes"][1]["counts"], "one shot: s's count cells")
    same(stats, got["nodes"][1]["children"][0][:, :, 0], "one shot: the stats child")


def test_index_rejections(W):
    from searchlite_amd import _native as N, aggs as A, searcher
    ix, q = W["ix"], (W["offs"], W["terms"], W["w"])

    def refused(request, code, word, fields=None, patch=None):
        plan = A.agg_spec(request, fields or W["agg_fields"])
        if patch:
            patch(plan)
        with pytest.raises(N.SlgError) as ei:
            ix.prepare(*q, 5, aggs=plan)
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    refused({"s": SIG("tag", 5)}, N.ERR_INVALID, "unknown agg field", fields=dict(W["agg_fields"], tag={"id": 999, "keys": TAG_KEYS}))
    wrong = dict(W["agg_fields"], tag={"id": W["agg_fields"]["x"]["id"], "keys": TAG_KEYS})
    refused({"r": RARE("tag", 5)}, N.ERR_INVALID, "numeric field", fields=wrong)

    def unknown_filter(plan):
        plan.term_buckets["spec"].nodes[0].background_filter = 999
    refused({"s": SIG("tag", 5)}, N.ERR_INVALID, "unknown filter id", patch=unknown_filter)
    for bad in ([0, 1, 2, 3, 4, 4], [0, 1, 2, 3, 4, 6]):  # a repeat, a rank beyond the dictionary
        arr = np.array(bad, np.uint32)

        def patch(plan, arr=arr):
            plan.term_buckets["spec"].nodes[0].ord_rank = arr.ctypes.data
        refused({"s": SIG("tag", 5)}, N.ERR_INVALID, "permutation", patch=patch)
    # a column without a row for a segment added later is refused by name (agg_field_rows): covered by the lifecycle
    # tests of every registered column; here: the batch does not run sharded
    b = ix.prepare(*q, 5, aggs=A.agg_spec({"s": SIG("tag", 5)}, W["agg_fields"]))
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
    # the calls on a batch of another kind
    with ix.prepare(*q, 5) as plain:
        plain.run()
        lib = plain._lib
        assert lib.slg_batch_term_buckets_layout(plain._h, None) == N.ERR_INVALID
        assert lib.slg_batch_fetch_term_buckets(plain._h, None, None, None, None, None, None, None) == N.ERR_INVALID
    # the other batch kinds take no term bucket spec
    with pytest.raises(N.SlgError) as ei:
        ix.prepare(*q, 5, aggs=A.agg_spec({"s": SIG("tag", 5)}, W["agg_fields"]), cursors=[None] * NQ)
    assert ei.value.code == N.ERR_UNSUPPORTED


# ---- 9. against the reference outright: one segment ---------------------------------------------------------------------------
def test_one_segment_equals_the_reference(gpu, oracle):
    """on one segment the device's counting is the reference's: both modes of the restatement agree and the device
    equals them.  Every doc has a value and the query matches every doc: doc_count == bg_count and every bucket's
    foreground is its background, so every score is exactly 1.0 and the order is (count desc, key bytes asc)"""
    from searchlite_amd import aggs as A
    rng = np.random.default_rng(5)
    n = 90
    seg = random_segment(rng, n, 3, 4, k1=0.9, b=0.4)
    seg = _append_lists(seg, [(np.arange(n), np.ones(n))])  # (term 3: every doc)
    keys = ["d", "é", "b", "ab", "Z", "c", "aa"]
    per_key = [10, 10, 15, 15, 15, 12, 13]  # (count ties: d = é, b = ab = Z; broken by key bytes)
    flat = [k for k, c in zip(keys, per_key) for _ in range(c)]
    assert len(flat) == n
    col = [[[flat[int(i)]] * (2 if d % 7 == 0 else 1) for d, i in enumerate(rng.permutation(n))]]  # (some hold it twice)
    cols, n_docs, hits = {"f": col}, [n], [(0, d) for d in range(n)]
    ix = gpu.GpuIndex([seg])
    try:
        fields = {"f": {"id": register_keyword(ix, col, keys), "keys": keys}}
        offs, terms, w = np.array([0, 1], np.uint32), np.array([[3]], np.uint32), np.ones(1, np.float32)
        for size in (2, 4, 7):
            req = {"s": SIG("f", size), "r": RARE("f", size, max_doc_count=30)}
            plan = A.agg_spec(req, fields)
            with ix.prepare(offs, terms, w, 3, aggs=plan) as b:
                lay = b.term_buckets_layout()
                b.run()
                assert b.matched_counts().tolist() == [n]
                got = A.shape_term_buckets(plan, lay, b.term_buckets(), 0)
            for name, body in req.items():
                ref = R.strip(R.respond(body, cols, n_docs, None, {}, hits, True))
                dev = R.strip(R.respond(body, cols, n_docs, None, {}, hits, False))
                assert ref == dev == got[name], (name, size)
                if name == "s":
                    assert all(R.score_bits(b_["score"]) == R.score_bits(1.0) for b_ in ref["buckets"])
                    cs = [b_["doc_count"] for b_ in ref["buckets"]]
                    assert cs == sorted(cs, reverse=True)  # equal scores: count desc ...
        full = R.strip(R.respond(SIG("f", 7), cols, n_docs, None, {}, hits, True))["buckets"]
        ties = [(a, b_) for a, b_ in zip(full, full[1:]) if a["doc_count"] == b_["doc_count"]]
        assert len(ties) == 3 and all(a["key"].encode() < b_["key"].encode() for a, b_ in ties)  # ... then key bytes asc
    finally:
        ix.close()
