"""Field-sorted search on the device (slg_index_add_sort_field_* + slg_batch_prepare_sorted).

Expected rows: the oracle run with k >= the number of docs returns every accepted doc with its exact score
(the set and the bits the reference's collector path sees); those hits are sorted in Python by a restatement
of SortKey::cmp (query/sort.rs:80-123: parts in order, Missing after every value in both orders, then
segment asc, doc asc) and cut at k.  Bar: the same (segment, doc) sequence, scores bit-identical when a part
is `_score` and 0.0 otherwise (ScoreMode::MatchOnly), matched = the accepted count (total_matches).
"""
import copy
import math
import struct

import numpy as np
import pytest

from tests.test_sort_keys import pick, total_key
from tests.util import load_golden, random_queries, random_segment

pytestmark = pytest.mark.gpu

NO_TERM = 0xFFFFFFFF


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return sa


def f64(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


NANS = [f64(0x7FF8000000000000), f64(0xFFF8000000000000), f64(0x7FF0000000000001)]


def score_key(x):
    b = struct.unpack("<i", struct.pack("<f", float(x)))[0]
    return b ^ ((b >> 31) & 0x7FFFFFFF)  # f32::total_cmp as a signed integer order


def part_key(part, order, seg, doc, score, fields):
    """one SortKeyPart as a tuple that orders like SortKeyPart::cmp"""
    if part == "_score":
        k = score_key(score)
        return (0, -k if order == "desc" else k)
    values, is_float = fields[part]
    v = pick(values[seg][doc], order)
    if v is None:
        return (1, 0)  # Missing: Greater than any value in both orders, Equal to Missing
    k = total_key(v, is_float)
    return (0, -k if order == "desc" else k)


def expected_rows(all_hits, sort, fields):
    """all_hits = oracle (doc, seg, score, count) with k >= docs -> per query [(seg, doc, score)] sorted"""
    doc, seg, score, count = all_hits
    rows = []
    for q in range(len(count)):
        hits = [(int(seg[q, i]), int(doc[q, i]), score[q, i]) for i in range(int(count[q]))]
        hits.sort(key=lambda h: tuple(part_key(p, o, h[0], h[1], h[2], fields) for p, o in sort) + (h[0], h[1]))
        rows.append(hits)
    return rows


def check(got, rows, k, sort, what=""):
    doc, seg, score, count, matched = got
    has_score = any(p == "_score" for p, _ in sort)
    for q, hits in enumerate(rows):
        n = min(len(hits), k)
        assert int(matched[q]) == len(hits), f"{what} q{q}: matched {int(matched[q])} != {len(hits)}"
        assert int(count[q]) == n, f"{what} q{q}: count {int(count[q])} != {n}"
        want_sd = [(h[0], h[1]) for h in hits[:n]]
        got_sd = list(zip(seg[q, :n].tolist(), doc[q, :n].tolist()))
        if got_sd != want_sd:
            i = next(i for i in range(n) if got_sd[i] != want_sd[i])
            raise AssertionError(f"{what} q{q}: first difference at rank {i}: {got_sd[i]} != {want_sd[i]}")
        if has_score:
            want = np.array([h[2] for h in hits[:n]], dtype=np.float32).view(np.uint32)
            assert np.array_equal(score[q, :n].view(np.uint32), want), f"{what} q{q}: scores differ"
        else:
            assert not score[q, :n].view(np.uint32).any(), f"{what} q{q}: MatchOnly scores must be 0.0"


def tombstoned(seg, rng, frac):
    s = copy.copy(seg)
    dead = rng.random(seg.n_docs) < frac
    s.deleted = np.packbits(dead, bitorder="little")
    s.docs = float(seg.n_docs - int(dead.sum()))
    return s


def make_fields(rng, segs):
    """three sort fields: i64 with extremes and Missing docs, f64 with NaN / -0.0 / inf and multi-valued docs,
    and a low-cardinality i64 (8 values) whose ties cross every k boundary"""
    i64_pool = [0, 1, -1, 7, -7, 100, -(1 << 63), (1 << 63) - 1]
    f64_pool = [0.0, -0.0, 1.5, -1.5, 3.0, math.inf, -math.inf] + NANS
    fi, ff, fl = [], [], []
    for s in segs:
        n = s.n_docs
        fi.append([[i64_pool[j] for j in rng.integers(0, len(i64_pool), int(rng.integers(0, 3)))] for _ in range(n)])
        ff.append([[f64_pool[j] for j in rng.integers(0, len(f64_pool), int(rng.integers(0, 4)))] for _ in range(n)])
        fl.append([[int(rng.integers(0, 8))] for _ in range(n)])
    return {"i64": (fi, False), "f64": (ff, True), "low": (fl, False)}


@pytest.fixture(scope="module")
def world(gpu, oracle):
    rng = np.random.default_rng(2024)
    segs = [random_segment(rng, 3000, 60, 25, k1=0.9, b=0.4), random_segment(rng, 1500, 60, 25, k1=0.9, b=0.4),
            random_segment(rng, 800, 60, 25, k1=0.9, b=0.4)]
    segs[0] = tombstoned(segs[0], rng, 0.1)
    segs[2] = tombstoned(segs[2], rng, 0.2)
    offs, terms, w = random_queries(rng, 24, 3, 60, n_segs=3, weights=True)
    w[::5] -= 1.5  # some negative weights
    terms[-3:, :] = NO_TERM  # the last query matches nothing
    fields = make_fields(rng, segs)
    ix = gpu.GpuIndex(segs)
    ids = {name: ix.add_sort_field(vals, np.float64 if is_f else np.int64) for name, (vals, is_f) in fields.items()}
    k_all = sum(s.n_docs for s in segs)
    all_hits = oracle.search_batch(segs, offs, terms, w, k_all, strategy=oracle.BM25)
    yield dict(ix=ix, segs=segs, offs=offs, terms=terms, w=w, fields=fields, ids=ids, all=all_hits, k_all=k_all)
    ix.close()


SPECS = {
    "low_asc": [("low", "asc")],
    "i64_desc": [("i64", "desc")],
    "f64_desc_score": [("f64", "desc"), ("_score", "desc")],
    "score_first": [("_score", "desc"), ("low", "asc")],
    "four_score_last": [("low", "desc"), ("f64", "asc"), ("i64", "asc"), ("_score", "asc")],
}


def ids_of(sort, ids):
    return [(p if p == "_score" else ids[p], o) for p, o in sort]


@pytest.mark.parametrize("k", [1, 11, 400, 5000, 20001])
@pytest.mark.parametrize("spec", list(SPECS))
def test_sorted_rows_match_sortkey_order(gpu, world, spec, k):
    sort = SPECS[spec]
    W = world
    rows = expected_rows(W["all"], sort, W["fields"])
    for strat in (gpu.Wand, gpu.Bm25):
        got = W["ix"].search_sorted(W["offs"], W["terms"], W["w"], k, ids_of(sort, W["ids"]), strategy=strat)
        check(got, rows, k, sort, f"{spec} k={k} strategy={strat}")


def test_filter_and_min_match(gpu, world, oracle):
    W = world
    rng = np.random.default_rng(7)
    masks = [rng.random(s.n_docs) < 0.5 for s in W["segs"]]
    fid = W["ix"].add_filter(masks)
    nq = len(W["offs"]) - 1
    qf = np.where(np.arange(nq) % 2 == 0, fid, -1).astype(np.int32)
    sort = [("low", "asc"), ("_score", "desc")]
    want = oracle.search_batch_filtered(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], qf, {fid: masks},
                                        strategy=oracle.BM25)
    got = W["ix"].search_sorted(W["offs"], W["terms"], W["w"], 11, ids_of(sort, W["ids"]), q_filter=qf)
    check(got, expected_rows(want, sort, W["fields"]), 11, sort, "filter")
    mm = np.where(np.arange(nq) % 3 == 0, 2, 0).astype(np.uint32)
    want = oracle.search_batch_min_match(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], mm,
                                         strategy=oracle.BM25, q_filter=qf, filters={fid: masks})
    got = W["ix"].search_sorted(W["offs"], W["terms"], W["w"], 400, ids_of(sort, W["ids"]), q_filter=qf,
                                q_min_match=mm)
    check(got, expected_rows(want, sort, W["fields"]), 400, sort, "min_match")
    W["ix"].remove_filter(fid)


def test_flat_and_two_level_plans(gpu, world, oracle):
    W = world
    nq = len(W["offs"]) - 1
    sort = [("_score", "desc"), ("i64", "asc")]
    flat = dict(q_plan=np.full(nq, 1, np.int32), q_tie=np.full(nq, 0.25, np.float32))
    want = oracle.search_batch(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], strategy=oracle.BM25, **flat)
    got = W["ix"].search_sorted(W["offs"], W["terms"], W["w"], 11, ids_of(sort, W["ids"]), **flat)
    check(got, expected_rows(want, sort, W["fields"]), 11, sort, "flat DisMax")
    two = dict(q_nleaves=np.full(nq, 3, np.uint32), q_plan=np.zeros(nq, np.int32),
               q_leaf_offsets=(np.arange(nq + 1) * 3).astype(np.uint32),
               leaf_group=np.tile(np.array([0, 0, 1], np.uint32), nq),
               q_group_offsets=(np.arange(nq + 1) * 2).astype(np.uint32),
               group_plan=np.tile(np.array([1, 0], np.int32), nq),
               group_tie=np.tile(np.array([0.3, 0.0], np.float32), nq))
    want = oracle.search_batch(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], strategy=oracle.BM25, **two)
    got = W["ix"].search_sorted(W["offs"], W["terms"], W["w"], 400, ids_of(sort, W["ids"]), **two)
    check(got, expected_rows(want, sort, W["fields"]), 400, sort, "two-level plan")


@pytest.mark.parametrize("n_terms", [9, 32])
def test_many_term_queries(gpu, oracle, n_terms):
    rng = np.random.default_rng(300 + n_terms)
    segs = [random_segment(rng, 2000, 80, 30, k1=0.9, b=0.4), random_segment(rng, 900, 80, 30, k1=0.9, b=0.4)]
    offs, terms, w = random_queries(rng, 8, n_terms, 80, n_segs=2, weights=True)
    fields = make_fields(rng, segs)
    sort = [("f64", "asc"), ("_score", "desc")]
    with gpu.GpuIndex(segs) as ix:
        fid = ix.add_sort_field(fields["f64"][0], np.float64)
        want = oracle.search_batch(segs, offs, terms, w, 2900, strategy=oracle.BM25)
        for k in (11, 1001):
            got = ix.search_sorted(offs, terms, w, k, [(fid, "asc"), ("_score", "desc")])
            check(got, expected_rows(want, sort, fields), k, sort, f"{n_terms} terms k={k}")


def test_lifecycle_and_errors(gpu, oracle):
    from searchlite_amd import _native as N
    rng = np.random.default_rng(11)
    segs = [random_segment(rng, 1200, 40, 20, k1=0.9, b=0.4), random_segment(rng, 700, 40, 20, k1=0.9, b=0.4)]
    offs, terms, w = random_queries(rng, 12, 3, 40, n_segs=2, weights=True)
    fields = make_fields(rng, segs)
    sort = [("low", "asc"), ("_score", "desc")]
    with gpu.GpuIndex([copy.copy(s) for s in segs]) as ix:
        fid = ix.add_sort_field(fields["low"][0], np.int64)
        run = lambda f, t=terms: ix.search_sorted(offs, t, w, 11, [(f, "asc"), ("_score", "desc")])
        check(run(fid), expected_rows(oracle.search_batch(segs, offs, terms, w, 1900, strategy=oracle.BM25), sort,
                                      fields), 11, sort, "fresh")
        # update_deleted keeps the columns
        dead = rng.random(segs[0].n_docs) < 0.3
        bm = np.packbits(dead, bitorder="little")
        ix.update_deleted(0, bm, segs[0].n_docs - int(dead.sum()))
        cur = [tombstoned(segs[0], np.random.default_rng(0), 0.0), segs[1]]
        cur[0].deleted, cur[0].docs = bm, float(segs[0].n_docs - int(dead.sum()))
        check(run(fid), expected_rows(oracle.search_batch(cur, offs, terms, w, 1900, strategy=oracle.BM25), sort,
                                      fields), 11, sort, "after update_deleted")
        # a segment added after the field: the field has no column for it
        extra = random_segment(rng, 500, 40, 20, k1=0.9, b=0.4)
        ix.add_segment(extra)
        terms3 = np.concatenate([terms, terms[:, :1]], axis=1)
        with pytest.raises(N.SlgError) as ei:
            run(fid, terms3)
        assert ei.value.code == N.ERR_INVALID
        vals3 = fields["low"][0] + [[[int(x)] for x in rng.integers(0, 8, extra.n_docs)]]
        fid2 = ix.add_sort_field(vals3, np.int64)
        assert fid2 > fid
        segs3 = cur + [extra]
        fields3 = {"low": (vals3, False)}
        check(run(fid2, terms3), expected_rows(oracle.search_batch(segs3, offs, terms3, w, 2400, strategy=oracle.BM25),
                                               sort, fields3), 11, sort, "after add_segment")
        # remove_segment drops that segment's column
        ix.remove_segment(0)
        segs2 = segs3[1:]
        fields2 = {"low": (vals3[1:], False)}
        terms2 = terms3[:, 1:].copy()
        check(run(fid2, terms2), expected_rows(oracle.search_batch(segs2, offs, terms2, w, 1200,
                                                                   strategy=oracle.BM25), sort, fields2), 11, sort,
              "after remove_segment")
        # ids are never handed out again; a removed id is unknown
        ix.remove_sort_field(fid2)
        fid3 = ix.add_sort_field(fields2["low"][0], np.int64)
        assert fid3 not in (fid, fid2)
        for stale in (fid, fid2, 12345):
            with pytest.raises(N.SlgError) as ei:
                run(stale, terms2)
            assert ei.value.code == N.ERR_INVALID
        with pytest.raises(N.SlgError) as ei:  # more parts than SLG_MAX_SORT_PARTS
            ix.search_sorted(offs, terms2, w, 11, [(fid3, "asc")] * 4 + [("_score", "desc")])
        assert ei.value.code == N.ERR_UNSUPPORTED
        with pytest.raises(N.SlgError) as ei:
            ix.remove_sort_field(fid2)
        assert ei.value.code == N.ERR_INVALID
        b = ix.prepare(offs, terms2, w, 11)  # a batch without a sort spec has no matched counts
        try:
            b.run()
            with pytest.raises(N.SlgError):
                b.matched_counts()
        finally:
            b.close()


def test_recipes_by_total_time_asc(gpu, oracle):
    """recipes/queries/collapse-quick-by-cuisine.json's sort (total_time_minutes asc) over the reference's
    example corpus: 59 distinct values over 300 docs, so the k-th hit sits in a run of ties."""
    import os
    segs, z = load_golden("recipes.npz")
    col = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recipes_sort.npz"))
    offs, vals = col["total_time_minutes_offsets"], col["total_time_minutes"]
    per_doc = [[int(v) for v in vals[offs[d]:offs[d + 1]]] for d in range(segs[0].n_docs)]
    fields = {"ttm": ([per_doc], False)}
    qo, qt, qw = z["q_offsets"], z["q_terms"], z["q_weights"]
    want = oracle.search_batch(segs, qo, qt, qw, segs[0].n_docs, strategy=oracle.WAND)
    with gpu.GpuIndex(segs) as ix:
        fid = ix.add_sort_field([(offs, vals)], np.int64)
        for sort in ([("ttm", "asc")], [("ttm", "asc"), ("_score", "desc")]):
            for k in (11, 101):
                got = ix.search_sorted(qo, qt, qw, k, [(fid if p == "ttm" else p, o) for p, o in sort])
                check(got, expected_rows(want, sort, fields), k, sort, f"recipes {sort} k={k}")
