"""The CPU half of tests/test_gpu_vector_edges.py and tests/test_gpu_hybrid_edges.py: the worlds of
tests/vector_edge_worlds.py hold what the device cases rest on.  Counts are recomputed from the constants the worlds
module copies from slg_vsearch.hpp / slg_hybrid.hpp and compared with those headers' text, so a changed constant
fails here instead of silently emptying a device case."""
import os
import re

import numpy as np
import pytest

from tests import hybrid_ref as R
from tests import test_gpu_vector_search as V
from tests import vector_edge_worlds as E

F32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "searchlite_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _same_rows(a, b):
    """two V.reference results, bit for bit"""
    assert len(a) == len(b)
    for (ra, ta, ma), (rb, tb, mb) in zip(a, b):
        assert ta == tb and len(ra) == len(rb)
        for x, y in zip(ra, rb):
            assert x[:2] == y[:2] and F32(x[2]).tobytes() == F32(y[2]).tobytes() and F32(x[3]).tobytes() == F32(y[3]).tobytes()
        assert [sorted(m) for m in ma] == [sorted(m) for m in mb]
        for m1, m2 in zip(ma, mb):
            assert all(F32(m1[key]).tobytes() == F32(m2[key]).tobytes() for key in m1)


def test_constants_are_the_headers():
    hpp, hy = _src("slg_vsearch.hpp"), _src("slg_hybrid.hpp")
    for name, val in (("kVsTileDocs", E.TILE_DOCS), ("kVsTileQ", E.TILE_Q), ("kVsKc", E.KC), ("kVsRow", E.ROW),
                      ("kVsSmallK", E.SMALL_K), ("kVsBufCap", E.BUF_CAP), ("kVsBufCapNarrow", E.BUF_CAP_NARROW),
                      ("kVsSortCap", E.SORT_CAP)):
        assert re.search(rf"constexpr uint32_t {name} = {val};", hpp), name
    assert re.search(rf"constexpr uint32_t kHyThreads = {E.HY_THREADS};", hy)
    assert re.search(rf"constexpr uint32_t kHySpanMax = {E.HY_SPAN_MAX};", hy)
    # the host rules the worlds module restates, as the host files spell them
    vs, hyh = _src("slg_vsearch.hip"), _src("slg_hybrid.hip")
    assert "std::min<uint32_t>(n_tiles, (slg::kVsSortCap - slg::kVsSmallK) / slg::kVsSmallK)" in vs
    assert "chunk_docs = ((slg::kVsSortCap - K) / slg::kVsTileDocs) * slg::kVsTileDocs;" in vs
    assert "const uint32_t P = slg::vs_pow2(NC * K);" in vs and "P > slg::kVsSortCap ? 0 : (size_t)P * 8" in vs
    assert "((uintptr_t)a.qvecs & 15) == 0" in vs
    assert f"while (span > 64 && slots / span < {E.HY_MIN_GROUPS}) span >>= 1;" in hyh
    assert "std::min<uint32_t>(span, slg::kHyThreads)" in hyh
    # the dispatch of hy_score_rows the row-chunk dims sit around
    assert "(cl.dim & 3u) != 0 || cl.dim > 768u" in hy and "cl.dim <= 256u" in hy and "cl.dim <= 512u" in hy


def test_big_world_counts():
    total = sum(E.BIG_DOCS)
    assert total == 3 * 32_640 + 129 == 98_049 and 32_640 == 255 * E.TILE_DOCS
    assert E.n_tiles(total) == 767 and total - 766 * E.TILE_DOCS == 1           # the final tile holds one doc
    assert E.BIG_DOCS[0] % E.TILE_DOCS == 80                                      # the boundary lies inside a tile
    assert E.min_tiles_per_block(total) == 4 >= 3
    for n_cu in (1, 64, 104, 256, 304, 10_000):
        for cand in (1, 32, 33, 64):
            n_chunks, tpb = E.topk_grid(total, 3, cand, n_cu)
            assert tpb >= 4 and n_chunks <= 255 and (n_chunks - 1) * tpb < 767 <= n_chunks * tpb
            if n_cu >= 256:  # an MI355X: 192 workgroups of 4 tiles, the last of 3
                assert (n_chunks, tpb, 767 - (n_chunks - 1) * tpb) == (192, 4, 3)
    assert E.store_steps(total, 65) == (16_256, 7) and E.store_steps(total, 4000) == (12_288, 8)
    # narrow and wide buffers both occur, and both sides of kVsSmallK
    assert E.scan_lds_bytes(E.BUF_CAP_NARROW) == 49_152 and 32 <= E.SMALL_K // 2 < 33 <= E.SMALL_K < 65
    for order in E.BIG_ORDERS:
        W = E.big_world(order)
        have = np.concatenate([st[1] != E.NOVEC for st in W.stores])
        assert 0.08 < 1 - have.mean() < 0.12 and have[0] and have[-1]
        assert W.live(0, 1, E.BIG_DOCS[1] - 1) and sum(len(d) for d in W.dels.values()) == 9
        assert W.n_live_vectors() > 4000


def test_big_world_orders():
    """ascending: every doc's score exceeds all before it; descending: none; tied: one value.  Under the negative
    boost of query 2 ascending and descending swap."""
    for order in E.BIG_ORDERS:
        W = E.big_world(order)
        qv, boost, lists = E.big_lists(order)
        assert boost[:, 0].tolist() == [1.0, 2.0, -1.0]
        for q in range(3):
            sc, sg, dc = lists[q][0]
            assert len(sc) == W.n_live_vectors()
            flat = sg * E.BIG_DOCS[0] + dc
            by_flat = sc[np.argsort(flat)]
            d = np.diff(by_flat.astype(np.float64))
            rising = (order == "asc") != (boost[q, 0] < 0)
            if order == "tied":
                assert np.all(d == 0) and np.all(np.diff(flat) > 0)
            else:
                assert np.all(d > 0) if rising else np.all(d < 0)
                assert len(np.unique(sc)) == len(sc)


@pytest.mark.parametrize("order", ("asc", "desc", "perm", "tied"))
def test_exact_worlds_are_exact(oracle, order):
    """a 300-doc exact world: the oracle's scores, the vectorised reference's and the closed form round(v * x) * boost
    agree bit for bit for all four boosts; and so do whole references (rows, totals, lists)"""
    W = E.exact_world((170, 130), 8, order, seed=1, dels={0: {4, 9}, 1: {0}}, zeros=(7, 200))
    qv, boost = E.exact_queries(8, 8)
    assert sorted(set(boost[:, 0].tolist())) == [-2.0, -1.0, 1.0, 2.0]
    live = lambda s, d: W.live(0, s, d)
    for q in range(8):
        ents = V._clause_scores(oracle, W.stores, qv[q], boost[q, 0], live)
        sc, sg, dc = E.clause_scores_fast(W.stores, qv[q], boost[q, 0], W.live_masks)
        closed = E.closed_form_scores(W, qv, boost, q)
        assert len(ents) == len(sc) == len(closed) == W.n_live_vectors()
        for (v, s, d), v2, s2, d2 in zip(ents, sc, sg, dc):
            assert (s, d) == (int(s2), int(d2))
            assert F32(v).tobytes() == F32(v2).tobytes() == closed[(s, d)].tobytes()
        if order != "tied":
            vals = [float(v) for v, s, d in ents if (s, d) not in ((0, 7), (1, 30))]
            assert len(set(vals)) == len(vals)
    a = np.zeros((8, 1), F32)
    for cand in (8, 100):
        _same_rows(V.reference(oracle, [W.stores], [0], [0], qv, a, boost, cand, 12, W.live),
                   E.reference_from_lists(E.sorted_lists([W.stores], [0], qv, boost, W.live_masks), [0], [0], a, cand, 12))


@pytest.mark.parametrize("metric", (0, 1))
def test_vectorised_reference_equals_the_oracle_backed_one(oracle, metric):
    """random vectors, both metrics, two clauses over two fields, a segment without the second field, alphas"""
    rng = np.random.default_rng(77 + metric)
    n_docs = (180, 120)
    fields = [[V._store(rng, n, 33, metric) for n in n_docs], [V._store(rng, n_docs[0], 7, 1 - metric), None]]
    W = E.VecWorld(n_docs, fields[0], {0: {1, 50}, 1: {119}})
    nq, cf = 5, [0, 1]
    qv = np.concatenate([rng.standard_normal((nq, 33)), rng.standard_normal((nq, 7))], axis=1).astype(F32)
    boost = (rng.random((nq, 2)) * 3 - 1).astype(F32)
    boost[0, 0] = 0.0
    alpha = rng.choice(np.array([0.0, 0.3, 1.0], F32), size=(nq, 2)).astype(F32)
    lists = E.sorted_lists(fields, cf, qv, boost, W.live_masks)
    metrics = [metric, 1 - metric]
    for cand in (10, 150):
        _same_rows(V.reference(oracle, fields, metrics, cf, qv, alpha, boost, cand, 20, W.live),
                   E.reference_from_lists(lists, metrics, cf, alpha, cand, 20))
    for q in range(nq):
        parts = [qv[q, :33], qv[q, 33:]]
        assert E.list_gap(lists[q], boost[q], 10) == V.boundary_gap(oracle, fields, cf, parts, boost[q], 10,
                                                                    lambda s, d: W.live(0, s, d))


def test_random_big_world_queries_keep_the_gap():
    qv, boost, lists = E.big_random_lists()
    for q in range(3):
        for cand in (32, 64):
            assert E.list_gap(lists[q], boost[q], cand) >= 1e-4
        assert len(lists[q][0][0]) == E.big_random_world().n_live_vectors() > 64


def test_query_and_doc_tile_worlds():
    assert E.QUERY_TILE_NQS == (15, 16, 17, 63, 64, 65, 129)
    assert {(n + E.TILE_Q - 1) // E.TILE_Q for n in E.QUERY_TILE_NQS} == {1, 2, 3}
    assert {n % 16 for n in E.QUERY_TILE_NQS} == {15, 0, 1}
    qv, boost = E.exact_queries(129, 8)
    assert len({(float(qv[q, 0]), float(boost[q, 0])) for q in range(129)}) == 129 and np.all(boost != 0)
    assert len(set(qv[:, 0].tolist())) == 129
    W = E.query_tile_world()
    assert W.total == 300 and len(W.n_docs) == 2 and W.n_live_vectors() > 100   # cand 8 and 100 both truncate
    assert E.DOC_TILE_TOTALS == (1, 127, 128, 129, 256, 257)
    for n in E.DOC_TILE_TOTALS:
        W = E.doc_tile_world(n)
        assert W.n_docs == [n] and E.n_tiles(n) == (n + 127) // 128 and 1 <= W.n_live_vectors() <= n
    W = E.doc_tile_world("3seg")
    assert np.cumsum(W.n_docs).tolist() == [64, 128, 129] and W.stores[1] is None and W.stores[0] and W.stores[2]
    assert W.stores[2][1][0] != E.NOVEC     # the doc alone in the second tile has a vector
    # cand 5 truncates every world but the one-doc one; cand 70 takes the store path
    assert E.doc_tile_world(127).n_live_vectors() > 70 > E.SMALL_K and E.doc_tile_world("3seg").n_live_vectors() < 70


def test_dim_step_worlds(oracle):
    assert set(E.DIM_STEPS[0]) == {31, 32, 33, 36, 63, 64, 65} and set(E.DIM_STEPS[1]) == {5, 31, 33, 36}
    assert any(d % 4 for d in E.DIM_STEPS[1]) and 36 % 4 == 0 and E.KC < 36 < 2 * E.KC
    for metric, dims in E.DIM_STEPS.items():
        for dim in dims:
            W, qv, boost = E.dim_world(dim, metric)
            assert qv.shape == (4, dim) and np.all(qv[:, -1] == E.DIM_TAIL[1][metric])
            for st in W.stores:
                assert st is None or np.all(st[2][:, -1] == E.DIM_ROW_TAIL[metric])
            lists = E.sorted_lists([W.stores], [0], qv, boost, W.live_masks)
            for q in range(4):
                assert min(E.list_gap(lists[q], boost[q], c) for c in (20, 70)) >= 1e-4
                # the tail's share of a score: dropping it moves every score by >= 0.02, 2000 x TOL
                cut = E.clause_scores_fast([None if st is None else (st[0], st[1], st[2][:, :-1]) for st in W.stores],
                                           qv[q, :-1], 1.0, W.live_masks)
                full = {(int(s), int(d)): float(v) for v, s, d in zip(*lists[q][0])}
                assert min(abs(full[(int(s), int(d))] - float(v)) for v, s, d in zip(*cut)) >= 0.02
                assert max(abs(v) for v in full.values()) < 4.0


def test_union_worlds():
    for nc, cand in E.UNION_CASES:
        assert E.blend_P(nc, cand) == 32_768 > E.SORT_CAP
        W, fields, cf, qv, alpha, boost, lists = E.union_world(nc, cand)
        assert len(cf) == nc and set(cf) == {0, 1} and np.all(boost == 40.0)
        for q in range(len(qv)):
            assert E.list_gap(lists[q], boost[q], cand) >= 1e-4
            assert all(len(l[0]) > cand for l in lists[q])      # every clause list is truncated
    assert E.blend_P(1, 10_000) == E.SORT_CAP                    # the largest case before this file: LDS
    assert [nc % 2 for nc, _ in E.UNION_CASES] == [0, 1]


def test_zero_and_nan_worlds(oracle):
    A, B, zeros = E.signed_zero_world()
    for f in zeros:
        s, d = f // 60, f % 60
        assert not A.stores[s][2][A.stores[s][1][d]].any()
    assert all(not st[2].any() for st in B.stores)
    ents = V._clause_scores(oracle, A.stores, np.eye(8, dtype=F32)[0], -1.0, lambda s, d: A.live(0, s, d))
    lead = [e for e in ents if e[0] == 0]
    assert len(lead) == 10 and ents[:10] == lead and all(np.signbit(e[0]) for e in lead)
    assert [(s, d) for _, s, d in lead] == [(f // 60, f % 60) for f in zeros] and all(e[0] < 0 for e in ents[10:])
    ents = V._clause_scores(oracle, B.stores, np.eye(8, dtype=F32)[0], 1.0, lambda s, d: True)
    assert all(e[0] == 0 and not np.signbit(e[0]) for e in ents)
    W = E.nan_world()
    q = np.eye(8, dtype=F32)[0]
    with np.errstate(invalid="ignore"):
        for f in E.NAN_FLATS:
            s, d = f // 80, f % 80
            row = W.stores[s][2][W.stores[s][1][d]]
            assert np.isinf(row[3]) and q[3] == 0 and np.isnan(np.dot(row, q))
    ents = V._clause_scores(oracle, W.stores, q, -1.0, lambda s, d: W.live(0, s, d))
    n = len(E.NAN_FLATS + E.ZERO_FLATS)
    assert [(s * 80 + d) for _, s, d in ents[:n]] == sorted(E.NAN_FLATS + E.ZERO_FLATS)
    assert all(e[0] == 0 and np.signbit(e[0]) for e in ents[:n]) and all(e[0] < 0 for e in ents[n:])
    assert 64 < W.n_live_vectors() <= 160


def test_row_chunk_world(oracle):
    assert E.CHUNK_DIMS == (252, 256, 260, 300, 512, 516, 764, 768, 772) and len(E.CHUNK_CASES) == 18
    chunks = lambda d: 0 if d % 4 or d > 768 else (d + 255) // 256    # hy_gather_kernel's dispatch
    assert [chunks(d) for d in E.CHUNK_DIMS] == [1, 1, 2, 2, 2, 3, 3, 3, 0]
    assert sum(1 for d in E.CHUNK_DIMS if chunks(d) and d % 256) == 5   # partial last chunks: 252, 260, 300, 516, 764
    W = E.chunk_world()
    assert sum(E.CHUNK_DOCS) == 300 and all(0.2 < 1 - h.mean() < 0.4 for h in W.have)
    # the crafted lists: one batch of at most 64 candidates, 7 / 1 / 61 of them with a vector, none deleted
    for name, (s, with_vec, without) in E.CHUNK_LISTS.items():
        seg, term, docs = W.lists[name]
        assert seg == s and len(docs) == with_vec + without <= 64 and int(W.have[s][docs].sum()) == with_vec
        assert not set(docs.tolist()) & W.dels[s]
        lo, hi = int(W.segs[s].term_offsets[term]), int(W.segs[s].term_offsets[term + 1])
        assert W.segs[s].doc_ids[lo:hi].tolist() == docs.tolist()
    assert [v % 4 for _, v, _ in E.CHUNK_LISTS.values()] == [3, 1, 1] and E.CHUNK_LISTS["m1"][1] == 1
    matched = R.matched(oracle, W.segs, *W.qs)
    for q, name in enumerate(E.CHUNK_LISTS):
        s, _, docs = W.lists[name]
        assert sorted((sg, d) for sg, d, _ in matched[q]) == [(s, int(d)) for d in docs]
    assert all(len(matched[q]) > E.CHUNK_CAND for q in range(3, E.CHUNK_NQ))


@pytest.mark.parametrize("dim,metric", E.CHUNK_CASES)
def test_row_chunk_cases_skip_nothing(oracle, dim, metric):
    """against the reference alone, with the vectors the device file uses: no query of a case has a boundary gap below
    GAP (the share left out of the order check is 0, within the 10 % test_gpu_hybrid enforces); tails as stated"""
    from tests.test_gpu_hybrid import GAP
    assert E.GAP == GAP
    W = E.chunk_world()
    stores, qv = E.chunk_field(oracle, dim, metric)
    assert np.all(qv[:, -4:] == E.CHUNK_Q_TAIL) and all(np.all(st[2][:, -4:] == E.CHUNK_ROW_TAIL[metric]) for st in stores)
    want = R.reference(oracle, W.segs, [stores], [0], *W.qs, E.CHUNK_K, qv, E.CHUNK_ALPHA, None, E.CHUNK_CAND, E.CHUNK_K)
    assert sum(w["gap"] < GAP for w in want) == 0
    # dropping the last four components moves a clause score by >= 0.1 (1e4 x TOL); scores stay small
    m = want[3]["maps"][0]
    cut = [None if st is None else (st[0], st[1], st[2][:, :-4]) for st in stores]
    sc, sg, dc = E.clause_scores_fast(cut, qv[3, :-4], 1.0)
    short = {(int(s), int(d)): float(v) for v, s, d in zip(sc, sg, dc)}
    assert min(abs(float(v) - short[key]) for key, v in m.items()) >= 0.1
    assert max(abs(float(v)) for w in want for v in w["maps"][0].values()) < 4.0


def test_multi_wave_worlds(oracle):
    from tests.test_gpu_hybrid import GAP
    W = E.wave_world()
    assert len(W.text_segs) == 2 and sum(E.WAVE_DOCS) == 41_000 and all(len(d) > 100 for d in W.dels.values())
    thresholds = {128: 262_144, 256: 524_288, 1024: 2_097_152}
    for span, nq in E.WAVE_CASES.items():
        assert E.hy_threshold(span) == thresholds[span]
        qs, qv, boost, want = E.wave_queries(oracle, span)
        slots = E.query_slots(W.text_segs, qs[0], qs[1])
        total = int(slots.sum())
        assert total >= 1.25 * thresholds[span] and E.hy_span(total) == span
        if span != 1024:
            assert total < E.hy_threshold(2 * span) and E.hy_span(total - 1) == span
        assert min(span, E.HY_THREADS) // 64 == {128: 2, 256: 4, 1024: 4}[span]
        # unequal regions, not multiples of 64; an empty query between two large ones
        assert slots[nq // 2] == 0 and min(slots[nq // 2 - 1], slots[nq // 2 + 1]) >= 41_000
        assert len(set(slots.tolist())) >= 4 and all(int(s) % 64 for s in slots if s)
        assert len({tuple(v) for v in qv.tolist()}) == nq and len(set(boost[:, 0].tolist())) == nq
        # the share of queries left out of the order check: none (10 % allowed)
        assert sum(w["gap"] < GAP for w in want) == 0 and want[nq // 2]["total"] == 0
        assert all(w["total"] >= E.WAVE_CAND for q, w in enumerate(want) if q != nq // 2)


def test_all_docs_reference_equals_hybrid_ref(oracle):
    """hybrid_reference_all_docs against tests/hybrid_ref.reference on a small all-docs world (same query shapes: the
    all-docs term alone, with a word, and no term)"""
    from tests.test_gpu_hybrid import _all_docs_world
    rng = np.random.default_rng(9)
    n_docs = [220, 140]
    segs, st0 = _all_docs_world(rng, n_docs, E.WAVE_VOCAB, E.WAVE_DIM)
    dels = {0: {3, 100}, 1: {139}}
    for s, sg in enumerate(segs):
        sg.set_deleted(sorted(dels[s]))
    W = E.VecWorld(n_docs, st0, dels)
    W.text_segs = segs
    T = E.WAVE_VOCAB
    terms = np.array([[T, T], [T, T], [4, 4], [E.NO_TERM, E.NO_TERM], [T, T], [0, 0]], np.uint32)
    qs = (np.array([0, 1, 3, 4, 6], np.uint32), terms, np.ones(6, F32))
    qv = V._unit(rng, 4, E.WAVE_DIM)
    boost = np.array([[1.0], [2.5], [1.0], [0.7]], F32)
    for cand, k in ((20, 11), (5, 30)):
        a = R.reference(oracle, segs, [st0], [0], *qs, k, qv, 0.5, boost, cand, k)
        b = E.hybrid_reference_all_docs(oracle, W, qs, k, qv, 0.5, boost, cand, k)
        for x, y in zip(a, b):
            assert x["total"] == y["total"] and x["gap"] == y["gap"] and x["near"] == y["near"]
            assert x["bm25"] == y["bm25"] and len(x["rows"]) == len(y["rows"])
            for r1, r2 in zip(x["rows"], y["rows"]):
                assert r1[:2] == r2[:2] and F32(r1[2]).tobytes() == F32(r2[2]).tobytes()
                assert (r1[3] is None) == (r2[3] is None) and (r1[3] is None or F32(r1[3]).tobytes() == F32(r2[3]).tobytes())
            assert x["maps"][0].keys() == y["maps"][0].keys()
            assert all(F32(x["maps"][0][key]).tobytes() == F32(y["maps"][0][key]).tobytes() for key in x["maps"][0])
