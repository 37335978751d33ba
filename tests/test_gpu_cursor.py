"""Cursor pagination on the device (slg_batch_prepare_after): per query the top k strictly after its cursor, in
score order (no sort spec) and in field sorts.

Expected rows: the oracle run with k >= the number of docs returns every accepted doc with its exact score;
those hits are ordered in Python by a restatement of SortKey::cmp (query/sort.rs:80-123; score order = score
desc by f32 total_cmp, then segment asc, doc asc).  The window of a cursor is every hit whose key is strictly
greater than the cursor's (the reference's accept(), api/reader.rs:3009-3036), cut at k.  Bar: the same
(segment, doc) sequence, scores bit-identical where scored (0.0 in a field sort without `_score`), matched = the
accepted docs after the cursor, seen = 1 exactly when an accepted doc has the cursor's key.
"""
import copy
import ctypes as C
import math
import struct

import numpy as np
import pytest

from tests.test_gpu_sort import make_fields, score_key, tombstoned
from tests.test_sort_keys import I64_MIN, f64, pick, total_key
from tests.util import random_queries, random_segment

pytestmark = pytest.mark.gpu

NO_TERM = 0xFFFFFFFF


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return sa


SPECS = {
    "score": None,  # score order: no sort spec
    "i64_asc": [("i64", "asc")],
    "f64_desc_score": [("f64", "desc"), ("_score", "desc")],
    "low_asc": [("low", "asc")],  # 8 values: long tie runs across segments
}


# ---- the reference's order, restated -------------------------------------------------------------------
def parts_of(sort):
    return [("_score", "desc")] if sort is None else sort


def key_of(sort, fields, values, seg, doc):
    """SortKey as a tuple that orders like SortKey::cmp; values: one per part (score, picked value or None)"""
    k = []
    for (p, o), v in zip(parts_of(sort), values):
        if p == "_score":
            s = score_key(v)
            k.append((0, -s if o == "desc" else s))
        elif v is None:
            k.append((1, 0))  # Missing after every value in both orders
        else:
            t = total_key(v, fields[p][1])
            k.append((0, -t if o == "desc" else t))
    return tuple(k) + (seg, doc)


class Hit:
    __slots__ = ("seg", "doc", "score", "values", "key")

    def __init__(self, sort, fields, seg, doc, score):
        self.seg, self.doc, self.score = seg, doc, score
        self.values = tuple(score if p == "_score" else pick(fields[p][0][seg][doc], o) for p, o in parts_of(sort))
        self.key = key_of(sort, fields, self.values, seg, doc)


def ordered_rows(all_hits, sort, fields):
    doc, seg, score, count = all_hits
    rows = []
    for q in range(len(count)):
        hits = [Hit(sort, fields, int(seg[q, i]), int(doc[q, i]), score[q, i]) for i in range(int(count[q]))]
        hits.sort(key=lambda h: h.key)
        rows.append(hits)
    return rows


def ids_of(sort, ids):
    return None if sort is None else [(p if p == "_score" else ids[p], o) for p, o in sort]


def cursor_of(h):
    return (h.values, h.seg, h.doc)


def check_row(got, q, rows, cur, k, sort, fields, seen=1, what=""):
    """cur: None (a first page) or (values, seg, doc)"""
    doc, seg, score, count, matched, got_seen = got
    after = rows if cur is None else [h for h in rows if h.key > key_of(sort, fields, *cur)]
    want = after[:k]
    n = len(want)
    assert int(got_seen[q]) == seen, f"{what} q{q}: seen {int(got_seen[q])} != {seen}"
    assert int(matched[q]) == len(after), f"{what} q{q}: matched {int(matched[q])} != {len(after)}"
    assert int(count[q]) == n, f"{what} q{q}: count {int(count[q])} != {n}"
    got_sd = list(zip(seg[q, :n].tolist(), doc[q, :n].tolist()))
    want_sd = [(h.seg, h.doc) for h in want]
    if got_sd != want_sd:
        i = next(i for i in range(n) if got_sd[i] != want_sd[i])
        raise AssertionError(f"{what} q{q}: first difference at rank {i}: {got_sd[i]} != {want_sd[i]}")
    if sort is None or any(p == "_score" for p, _ in sort):
        w = np.array([h.score for h in want], dtype=np.float32).view(np.uint32)
        assert np.array_equal(score[q, :n].view(np.uint32), w), f"{what} q{q}: scores differ"
    else:
        assert not score[q, :n].view(np.uint32).any(), f"{what} q{q}: MatchOnly scores must be 0.0"


def walk(ix, W, sort, rows, L, what, **kw):
    """page through every query: k = L + 1, the next cursor from row L - 1, stop when count <= L; the pages
    concatenated must be the whole expected order"""
    nq = len(rows)
    cursors = [None] * nq
    pages = [[] for _ in range(nq)]
    done = [False] * nq
    n_pages = 0
    while not all(done):
        got = ix.search_after(W["offs"], W["terms"], W["w"], L + 1, cursors, sort=ids_of(sort, W["ids"]), **kw)
        for q in range(nq):
            if done[q]:
                continue
            check_row(got, q, rows[q], cursors[q], L + 1, sort, W["fields"], what=f"{what} page {n_pages}")
            c = int(got[3][q])
            pages[q] += [(int(got[1][q, i]), int(got[0][q, i])) for i in range(min(c, L))]
            if c <= L:
                done[q] = True
            else:
                cursors[q] = cursor_of(rows[q][len(pages[q]) - 1])
        n_pages += 1
    for q in range(nq):
        assert pages[q] == [(h.seg, h.doc) for h in rows[q]], f"{what} q{q}: pages concatenated differ"


@pytest.fixture(scope="module")
def world(gpu, oracle):
    rng = np.random.default_rng(4242)
    segs = [random_segment(rng, 300, 60, 12, k1=0.9, b=0.4), random_segment(rng, 200, 60, 12, k1=0.9, b=0.4),
            random_segment(rng, 120, 60, 12, k1=0.9, b=0.4)]
    segs[0] = tombstoned(segs[0], rng, 0.1)
    segs[2] = tombstoned(segs[2], rng, 0.2)
    offs, terms, w = random_queries(rng, 12, 3, 60, n_segs=3, lo=8, weights=True)
    w[::5] -= 1.5  # some negative weights
    terms[-3:, :] = NO_TERM  # the last query matches nothing
    fields = make_fields(rng, segs)
    ix = gpu.GpuIndex(segs)
    ids = {name: ix.add_sort_field(vals, np.float64 if is_f else np.int64) for name, (vals, is_f) in fields.items()}
    k_all = sum(s.n_docs for s in segs)
    all_hits = oracle.search_batch(segs, offs, terms, w, k_all, strategy=oracle.BM25)
    masks = [rng.random(s.n_docs) < 0.6 for s in segs]
    fid = ix.add_filter(masks)
    nq = len(offs) - 1
    qf = np.where(np.arange(nq) % 2 == 0, fid, -1).astype(np.int32)
    filtered = oracle.search_batch_filtered(segs, offs, terms, w, k_all, qf, {fid: masks}, strategy=oracle.BM25)
    yield dict(ix=ix, segs=segs, offs=offs, terms=terms, w=w, fields=fields, ids=ids, all=all_hits, k_all=k_all,
               qf=qf, masks=masks, fid=fid, filtered=filtered)
    ix.close()


@pytest.mark.parametrize("L", [1, 10, 300])
@pytest.mark.parametrize("spec", list(SPECS))
def test_page_walk(gpu, world, spec, L):
    W, sort = world, SPECS[spec]
    walk(W["ix"], W, sort, ordered_rows(W["all"], sort, W["fields"]), L, f"{spec} L={L}")
    walk(W["ix"], W, sort, ordered_rows(W["filtered"], sort, W["fields"]), L, f"{spec} L={L} filtered",
         q_filter=W["qf"], strategy=gpu.Bm25)


@pytest.mark.parametrize("spec", ["score", "i64_asc"])
def test_page_walk_plans_and_min_match(gpu, world, oracle, spec):
    W, sort = world, SPECS[spec]
    nq = len(W["offs"]) - 1
    flat = dict(q_plan=np.full(nq, 1, np.int32), q_tie=np.full(nq, 0.25, np.float32))
    two = dict(q_nleaves=np.full(nq, 3, np.uint32), q_plan=np.zeros(nq, np.int32),
               q_leaf_offsets=(np.arange(nq + 1) * 3).astype(np.uint32),
               leaf_group=np.tile(np.array([0, 0, 1], np.uint32), nq),
               q_group_offsets=(np.arange(nq + 1) * 2).astype(np.uint32),
               group_plan=np.tile(np.array([1, 0], np.int32), nq),
               group_tie=np.tile(np.array([0.3, 0.0], np.float32), nq))
    for name, plan in (("flat DisMax", flat), ("two-level", two)):
        want = oracle.search_batch(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], strategy=oracle.BM25, **plan)
        walk(W["ix"], W, sort, ordered_rows(want, sort, W["fields"]), 10, f"{spec} {name}", **plan)
    mm = np.where(np.arange(nq) % 3 == 0, 2, 0).astype(np.uint32)
    want = oracle.search_batch_min_match(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], mm,
                                         strategy=oracle.BM25, q_filter=W["qf"], filters={W["fid"]: W["masks"]})
    walk(W["ix"], W, sort, ordered_rows(want, sort, W["fields"]), 10, f"{spec} min_match", q_filter=W["qf"],
         q_min_match=mm)


@pytest.mark.parametrize("n_terms", [9, 32])
def test_page_walk_many_term_queries(gpu, oracle, n_terms):
    rng = np.random.default_rng(500 + n_terms)
    segs = [random_segment(rng, 400, 80, 10, k1=0.9, b=0.4), random_segment(rng, 250, 80, 10, k1=0.9, b=0.4)]
    segs[1] = tombstoned(segs[1], rng, 0.15)
    offs, terms, w = random_queries(rng, 6, n_terms, 80, n_segs=2, weights=True)
    fields = make_fields(rng, segs)
    want = oracle.search_batch(segs, offs, terms, w, 650, strategy=oracle.BM25)
    with gpu.GpuIndex(segs) as ix:
        W = dict(offs=offs, terms=terms, w=w, fields=fields, ids={"i64": ix.add_sort_field(fields["i64"][0], np.int64)})
        for spec in ("score", "i64_asc"):
            sort = SPECS[spec]
            walk(ix, W, sort, ordered_rows(want, sort, fields), 10, f"{n_terms} terms {spec}")


@pytest.mark.parametrize("spec", list(SPECS))
def test_mixed_batch_first_pages_equal_the_plain_batch(gpu, world, spec):
    """queries without a cursor share the batch with cursor queries and get exactly the row of
    slg_batch_prepare_sorted (field sorts) or slg_search_batch (score order)"""
    W, sort = world, SPECS[spec]
    rows = ordered_rows(W["all"], sort, W["fields"])
    nq = len(rows)
    for k in (11, 300):
        cursors = [cursor_of(rows[q][len(rows[q]) // 3]) if q % 2 and rows[q] else None for q in range(nq)]
        got = W["ix"].search_after(W["offs"], W["terms"], W["w"], k, cursors, sort=ids_of(sort, W["ids"]))
        if sort is None:
            plain = W["ix"].search_batch(W["offs"], W["terms"], W["w"], k)
        else:
            plain = W["ix"].search_sorted(W["offs"], W["terms"], W["w"], k, ids_of(sort, W["ids"]))
        for q in range(nq):
            check_row(got, q, rows[q], cursors[q], k, sort, W["fields"], what=f"{spec} mixed k={k}")
            if cursors[q] is None:
                n = int(plain[3][q])
                assert int(got[3][q]) == n
                for a, b in zip(got[:3], plain[:3]):
                    assert np.array_equal(a[q, :n].view(np.uint32), b[q, :n].view(np.uint32)), f"{spec} q{q}"
                if sort is not None:
                    assert int(got[4][q]) == int(plain[4][q])


# a cursor key before every doc of the world: the largest score, or the first value of each part's order
ABOVE_ALL = {
    "score": ((math.inf,), 0, 0),
    "f64_desc_score": ((f64(0x7FFFFFFFFFFFFFFF), math.inf), 0, 0),  # the largest NaN: first in desc
    "low_asc": ((-1,), 0, 0),
    "i64_asc": ((I64_MIN,), 0, 0),  # (doc (0, 0) may itself hold I64_MIN: then it is the cursor doc)
}


@pytest.mark.parametrize("spec", list(SPECS))
def test_cursor_at_the_last_doc_and_above_every_doc(gpu, world, spec):
    W, sort = world, SPECS[spec]
    rows = ordered_rows(W["all"], sort, W["fields"])
    nq = len(rows)
    last = [cursor_of(rows[q][-1]) if rows[q] else None for q in range(nq)]
    got = W["ix"].search_after(W["offs"], W["terms"], W["w"], 11, last, sort=ids_of(sort, W["ids"]))
    for q in range(nq):
        if rows[q]:
            assert (int(got[3][q]), int(got[4][q]), int(got[5][q])) == (0, 0, 1), f"{spec} q{q}"
    top = ABOVE_ALL[spec]
    got = W["ix"].search_after(W["offs"], W["terms"], W["w"], 11, [top] * nq, sort=ids_of(sort, W["ids"]))
    plain = W["ix"].search_after(W["offs"], W["terms"], W["w"], 11, [None] * nq, sort=ids_of(sort, W["ids"]))
    ck = key_of(sort, W["fields"], *top)
    for q in range(nq):
        tied = any(h.key == ck for h in rows[q])
        check_row(got, q, rows[q], top, 11, sort, W["fields"], seen=int(tied), what=f"{spec} above every doc")
        if not tied:
            for a, b in zip(got[:5], plain[:5]):
                assert np.array_equal(a[q:q + 1].view(np.uint8), b[q:q + 1].view(np.uint8)), f"{spec} q{q}"


@pytest.mark.parametrize("k", [1, 11, 256, 257, 1001, 20001])
def test_score_order_every_k(gpu, world, k):
    W = world
    rows = ordered_rows(W["all"], None, W["fields"])
    nq = len(rows)
    for frac in (0.0, 0.5):
        cursors = [cursor_of(rows[q][int(len(rows[q]) * frac)]) if rows[q] else None for q in range(nq)]
        got = W["ix"].search_after(W["offs"], W["terms"], W["w"], k, cursors)
        for q in range(nq):
            check_row(got, q, rows[q], cursors[q], k, None, W["fields"], what=f"k={k} at {frac}")


@pytest.mark.parametrize("spec", ["score", "i64_asc"])
def test_stale_cursor_deleted_after_page_one(gpu, oracle, spec):
    rng = np.random.default_rng(77)
    segs = [random_segment(rng, 300, 40, 12, k1=0.9, b=0.4), random_segment(rng, 200, 40, 12, k1=0.9, b=0.4)]
    offs, terms, w = random_queries(rng, 8, 3, 40, n_segs=2, weights=True)
    fields = make_fields(rng, segs)
    sort = SPECS[spec]
    L = 5
    with gpu.GpuIndex([copy.copy(s) for s in segs]) as ix:
        ids = {"i64": ix.add_sort_field(fields["i64"][0], np.int64)}
        rows = ordered_rows(oracle.search_batch(segs, offs, terms, w, 500, strategy=oracle.BM25), sort, fields)
        nq = len(rows)
        got = ix.search_after(offs, terms, w, L + 1, [None] * nq, sort=ids_of(sort, ids))
        for q in range(nq):
            check_row(got, q, rows[q], None, L + 1, sort, fields, what=f"{spec} page 1")
        cursors = [cursor_of(rows[q][L - 1]) if len(rows[q]) > L else None for q in range(nq)]
        # delete every cursor doc (live_docs kept: the scores stay those of page 1)
        dead = [np.zeros(s.n_docs, bool) for s in segs]
        for c in cursors:
            if c is not None:
                dead[c[1]][c[2]] = True
        cur = [copy.copy(s) for s in segs]
        for s in range(2):
            bm = np.packbits(dead[s], bitorder="little")
            ix.update_deleted(s, bm, segs[s].docs)
            cur[s].deleted = bm
        rows2 = ordered_rows(oracle.search_batch(cur, offs, terms, w, 500, strategy=oracle.BM25), sort, fields)
        got = ix.search_after(offs, terms, w, L + 1, cursors, sort=ids_of(sort, ids))
        for q in range(nq):
            check_row(got, q, rows2[q], cursors[q], L + 1, sort, fields, seen=0 if cursors[q] else 1,
                      what=f"{spec} deleted cursor doc")


def f32_step(x, delta):
    b = struct.unpack("<I", struct.pack("<f", float(x)))[0]
    return struct.unpack("<f", struct.pack("<I", (b + delta) & 0xFFFFFFFF))[0]


def test_stale_cursor_filtered_out_and_score_one_ulp_off(gpu, world, oracle):
    W = world
    rows = ordered_rows(W["all"], None, W["fields"])
    nq = len(rows)
    cursors = [cursor_of(rows[q][len(rows[q]) // 2]) if rows[q] else None for q in range(nq)]
    # the cursor doc filtered out: every other doc passes
    masks = [np.ones(s.n_docs, bool) for s in W["segs"]]
    for c in cursors:
        if c is not None:
            masks[c[1]][c[2]] = False
    fid = W["ix"].add_filter(masks)
    try:
        qf = np.full(nq, fid, np.int32)
        want = ordered_rows(oracle.search_batch_filtered(W["segs"], W["offs"], W["terms"], W["w"], W["k_all"], qf,
                                                         {fid: masks}, strategy=oracle.BM25), None, W["fields"])
        got = W["ix"].search_after(W["offs"], W["terms"], W["w"], 11, cursors, q_filter=qf)
        for q in range(nq):
            check_row(got, q, want[q], cursors[q], 11, None, W["fields"], seen=0 if cursors[q] else 1,
                      what="filtered cursor doc")
    finally:
        W["ix"].remove_filter(fid)
    # the cursor's score one ulp off (smoke.rs:792: a tampered cursor)
    for delta in (1, -1):
        bad = [None if c is None else ((f32_step(c[0][0], delta),), c[1], c[2]) for c in cursors]
        got = W["ix"].search_after(W["offs"], W["terms"], W["w"], 11, bad)
        for q in range(nq):
            check_row(got, q, rows[q], bad[q], 11, None, W["fields"], seen=0 if bad[q] else 1,
                      what=f"score {delta:+d} ulp")


# ---- the reference's own cursor tests, on the device -------------------------------------------------------
def _rust_index(gpu, seg_docs):
    segs = []
    for docs in seg_docs:
        b = gpu.SegmentBuilder(["body"], k1=0.9, b=0.4)
        for ext, text in docs:
            b.add_document(ext, {"body": text})
        segs.append(b.build())
    ids = np.array([[s.term_id("body:rust") for s in segs]], dtype=np.uint32)
    return segs, np.array([0, 1], np.uint32), ids, np.ones(1, np.float32)


def _pages(ix, offs, terms, w, limit, values_of, sort=None, max_pages=10):
    """the reference's loop: `limit` hits a page, the next cursor from the page's last hit"""
    out, cur = [], None
    for _ in range(max_pages):
        doc, seg, score, count, matched, seen = ix.search_after(offs, terms, w, limit + 1, [cur], sort=sort)
        assert int(seen[0]) == 1
        n = int(count[0])
        out += [(int(seg[0, i]), int(doc[0, i]), score[0, i]) for i in range(min(n, limit))]
        if n <= limit:
            break
        s, d, sc = out[-1]
        cur = (values_of(s, d, sc), s, d)
    return out


def test_reference_cursor_paginates_ordered_hits(gpu):
    """smoke.rs:500-592: six docs over two segments, limit 2: three pages, six distinct docs"""
    segs, offs, terms, w = _rust_index(gpu, [[(str(i), "rust " * (6 - i)) for i in range(3)],
                                             [(str(i), "rust " * (6 - i)) for i in range(3, 6)]])
    with gpu.GpuIndex(segs) as ix:
        hits = _pages(ix, offs, terms, w, 2, lambda s, d, sc: (sc,))
    assert len(hits) == 6 and len({(s, d) for s, d, _ in hits}) == 6


def test_reference_cursor_orders_stably_across_segments(gpu):
    """smoke.rs:853-950: two segments x three equal "rust" docs page in (segment, doc) order"""
    segs, offs, terms, w = _rust_index(gpu, [[(f"doc-s0-{i}", "rust") for i in range(3)],
                                             [(f"doc-s1-{i}", "rust") for i in range(3)]])
    with gpu.GpuIndex(segs) as ix:
        hits = _pages(ix, offs, terms, w, 2, lambda s, d, sc: (sc,))
    assert [segs[s].ext_ids[d] for s, d, _ in hits] == [f"doc-s{s}-{i}" for s in range(2) for i in range(3)]


def test_reference_paginates_with_sorted_cursor_across_segments(gpu):
    """sorting.rs:227: rank asc over two segments, limit 2 -> 5, 10, 15, 20, 30"""
    segs, offs, terms, w = _rust_index(gpu, [[(f"r{v}", "rust paging") for v in (30, 10, 20)],
                                             [(f"r{v}", "rust paging") for v in (15, 5)]])
    rank = [[[int(e[1:])] for e in s.ext_ids] for s in segs]
    with gpu.GpuIndex(segs) as ix:
        fid = ix.add_sort_field(rank, np.int64)
        hits = _pages(ix, offs, terms, w, 2, lambda s, d, sc: (rank[s][d][0],), sort=[(fid, "asc")])
    assert [rank[s][d][0] for s, d, _ in hits] == [5, 10, 15, 20, 30]


# ---- errors and the one-shot form ----------------------------------------------------------------------------
def test_errors(gpu, world):
    from searchlite_amd import _native as N
    from searchlite_amd import searcher
    W = world
    nq = len(W["offs"]) - 1
    bad = N.SortCursor()
    bad.has_cursor, bad.missing_mask = 1, 2  # Missing on the `_score` part
    with pytest.raises(N.SlgError) as ei:
        W["ix"].search_after(W["offs"], W["terms"], W["w"], 11, [bad] * nq,
                             sort=ids_of([("i64", "asc"), ("_score", "desc")], W["ids"]))
    assert ei.value.code == N.ERR_INVALID
    bad = N.SortCursor()
    bad.has_cursor, bad.missing_mask = 1, 1  # score order: part 0 is the score
    with pytest.raises(N.SlgError) as ei:
        W["ix"].search_after(W["offs"], W["terms"], W["w"], 11, [bad] * nq)
    assert ei.value.code == N.ERR_INVALID
    lib = N.load()
    offs = np.ascontiguousarray(W["offs"], np.uint32)
    terms = np.ascontiguousarray(W["terms"], np.uint32)
    w = np.ascontiguousarray(W["w"], np.float32)
    h = lib.slg_batch_prepare_after(W["ix"]._h, nq, offs.ctypes.data, terms.ctypes.data, w.ctypes.data, None, None,
                                    None, None, 11, N.STRATEGY_WAND)
    assert h is None and N.last_error_code() == N.ERR_INVALID  # q_cursor NULL
    # a cursor batch does not run sharded (a cursor's segment_ord is index-global)
    b = W["ix"].prepare(W["offs"], W["terms"], W["w"], 11, cursors=[None] * nq)
    try:
        group = searcher.ShardGroup(W["ix"], 0, 1, searcher.shard_unique_id(), len(W["segs"]))
        try:
            with pytest.raises(N.SlgError) as ei:
                b.run_sharded(group)
            assert ei.value.code == N.ERR_UNSUPPORTED
            with pytest.raises(N.SlgError) as ei:
                b.fetch_sharded()
            assert ei.value.code == N.ERR_UNSUPPORTED
        finally:
            group.close()
    finally:
        b.close()
    b = W["ix"].prepare(W["offs"], W["terms"], W["w"], 11)  # a batch without cursors has no seen flags
    try:
        b.run()
        with pytest.raises(N.SlgError) as ei:
            b.cursor_seen()
        assert ei.value.code == N.ERR_INVALID
    finally:
        b.close()


def test_one_shot_form(gpu, world):
    """slg_search_batch_after: the prepared batch's rows, matched counts and seen flags in one call"""
    from searchlite_amd import _native as N
    from searchlite_amd.searcher import sort_cursor, sort_spec
    W = world
    sort = [("low", "asc"), ("_score", "desc")]
    rows = ordered_rows(W["all"], sort, W["fields"])
    nq = len(rows)
    cursors = [cursor_of(rows[q][len(rows[q]) // 4]) if rows[q] else None for q in range(nq)]
    sort_ids = ids_of(sort, W["ids"])
    want = W["ix"].search_after(W["offs"], W["terms"], W["w"], 11, cursors, sort=sort_ids)
    n_segs = len(W["segs"])
    terms = np.ascontiguousarray(W["terms"], np.uint32).reshape(-1, n_segs)
    w = np.ascontiguousarray(W["w"], np.float32)
    qs = (N.Query * nq)()
    for q in range(nq):
        a, b = int(W["offs"][q]), int(W["offs"][q + 1])
        qs[q] = N.Query(b - a, terms.ctypes.data + a * n_segs * 4, w.ctypes.data + a * 4)
    cur = (N.SortCursor * nq)(*[sort_cursor(c, sort_ids) for c in cursors])
    spec = sort_spec(sort_ids)
    out = [np.zeros((nq, 11), np.uint32), np.zeros((nq, 11), np.uint32), np.zeros((nq, 11), np.float32),
           np.zeros(nq, np.uint32), np.zeros(nq, np.uint64), np.zeros(nq, np.uint8)]
    N.check(N.load().slg_search_batch_after(W["ix"]._h, C.addressof(qs), nq, None, None, C.addressof(spec),
                                            C.addressof(cur), 11, N.STRATEGY_WAND, *[a.ctypes.data for a in out]))
    for a, b in zip(out, want):
        assert np.array_equal(a.view(np.uint8), np.asarray(b).view(np.uint8))
