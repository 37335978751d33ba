"""The CPU half of tests/test_gpu_vector_approx_edges.py: the worlds of tests/vector_approx_edge_worlds.py reach the
paths of vs_scan_bf16_kernel their cases name (counts recomputed from the constants the worlds modules copy from the
headers, compared with the headers' text), every value in them is a bf16 value, every score is exact in f32 in any
order, and each family of exact worlds moves under the defect it is meant to catch (A.first_pass_top's mutations).
The general-data worlds keep the band condition of their seeds."""
import os
import re

import numpy as np
import pytest

from tests import vector_approx_edge_worlds as A
from tests import vector_edge_worlds as E

F32, F64 = np.float32, np.float64
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "searchlite_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _all_bf16(W, qv, boost):
    return all(A.is_bf16(st[2]) for st in W.stores if st is not None) and A.is_bf16(qv) and A.is_bf16(boost)


def _exact_in_f32(W, qv, metric, below=2.0 ** 24):
    """every score of the world, as the first pass forms it (dot, norms, |x|^2 + |q|^2 - 2 x.q) and as the exact scan
    does (dot; sum (q - x)^2): f32 sums over two orders equal the f64 sums, so no addition rounds.  -> the largest
    magnitude met, in units of the values' grid (the caller states the grid)"""
    rows, ok = A.flat_view(W)
    X = rows[ok]
    top = 0.0
    for q in np.asarray(qv, F32):
        for order in (slice(None), slice(None, None, -1)):
            P = (X * q[None, :])[:, order]
            s32, s64 = np.cumsum(P, axis=1, dtype=F32)[:, -1], P.astype(F64).sum(1)
            assert np.array_equal(s32.astype(F64), s64)
            if metric == 1:
                sq = (X * X)[:, order]
                n32, n64 = np.cumsum(sq, axis=1, dtype=F32)[:, -1], sq.astype(F64).sum(1)
                qn32, qn64 = np.cumsum((q * q)[order], dtype=F32)[-1], float((q.astype(F64) ** 2).sum())
                assert np.array_equal(n32.astype(F64), n64) and float(qn32) == qn64
                D32 = ((n32 + qn32).astype(F32) - (F32(2.0) * s32).astype(F32)).astype(F32)
                d = (q[None, :] - X).astype(F32)
                assert np.array_equal(d.astype(F64), q.astype(F64)[None, :] - X.astype(F64))
                e = (d * d)[:, order]
                e32, e64 = np.cumsum(e, axis=1, dtype=F32)[:, -1], e.astype(F64).sum(1)
                assert np.array_equal(e32.astype(F64), e64) and np.array_equal(D32.astype(F64), e64)
                top = max(top, float(n64.max()), qn64, float(np.abs(2 * s64).max()), float(e64.max()))
            top = max(top, float(np.abs(P.astype(F64)).sum(1).max()))
    return top


def _model_is_the_reference(W, qv, boost, metric, R):
    """A.first_pass_top without a mutation picks the reference's best R, in order"""
    lists = E.sorted_lists([W.stores], [0], qv, boost, W.live_masks)
    tops = A.first_pass_top(A.flat_view(W), metric, qv, boost, R)
    for q, top in enumerate(tops):
        sc, sg, dc = lists[q][0]
        assert A.flat_keys(W, top) == [(int(s), int(d)) for s, d in zip(sg[:R], dc[:R])], q


def _moves(W, qv, boost, metric, R, mut, **kw):
    view = A.flat_view(W)
    a = A.first_pass_top(view, metric, qv, boost, R)
    b = A.first_pass_top(view, metric, qv, boost, R, mut=mut, **kw)
    return sum(not np.array_equal(x, y) for x, y in zip(a, b))


def test_constants_are_the_headers():
    hpp, hip = _src("slg_vsearch_approx.hpp"), _src("slg_vsearch.hip")
    assert re.search(rf"constexpr uint32_t kVaKc = {A.KC};", hpp)
    assert "return vs_scan_lds_bytes(topk, cap) + kVsTileDocs * 4;" in hpp
    assert "return (dim + kVaKc - 1) / kVaKc * kVaKc;" in hpp
    assert "if (k0 + kVaKc < dim_pad)" in hpp and "for (int h = 0; h < 2; h++) {  // two MFMA k-steps of 32" in hpp
    assert "base + i - p.tile_begin * kVsTileDocs" in hpp
    assert "(b + 0x7FFFu + ((b >> 16) & 1u)) >> 16" in hpp
    assert f"bf16 ? {A.BY_VGPRS}u : 3u" in hip
    assert "vc.q_floats % 4 == 0 && vc.coff[c] % 4 == 0 && ((uintptr_t)a.qvecs & 15) == 0" in hip
    assert "const VsPlan pl = vs_plan(ix, vc, R, refine != 0);" in hip      # the plan is cut for refine, not cand
    for cap in (E.BUF_CAP_NARROW, E.BUF_CAP):
        assert A.scan_lds_bytes(cap) == E.scan_lds_bytes(cap) + 512
        assert min(A.BY_VGPRS, (160 << 10) // A.scan_lds_bytes(cap)) == 2      # two resident workgroups per CU
    assert A.bf16_round(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -7], F32)).tolist() == \
        [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]                                 # ties to even


@pytest.mark.parametrize("metric", A.BIG_METRICS)
def test_big_world_counts_and_values(metric):
    total = sum(E.BIG_DOCS)
    assert total == 98_049 and E.n_tiles(total) == 767 and total - 766 * E.TILE_DOCS == 1
    assert E.BIG_DOCS[0] % E.TILE_DOCS == 80 and E.min_tiles_per_block(total) >= 4
    for n_cu in (1, 64, 104, 256, 304, 10_000):
        for R in A.BIG_TOPK:
            n_chunks, tpb = A.topk_grid(total, 3, R, n_cu)
            assert tpb >= 4 and n_chunks <= 255 and (n_chunks - 1) * tpb < 767 <= n_chunks * tpb
    assert {R <= E.SMALL_K // 2 for R in A.BIG_TOPK} == {True, False}           # both buffer caps
    assert [E.store_steps(total, R)[1] for _, R in A.BIG_STORE] == [7, 7, 8, 8]
    assert all(R > E.SMALL_K and c <= R for c, R in A.BIG_STORE) and any(c < R for c, R in A.BIG_STORE)
    qv, boost = A.big_queries(metric)
    assert boost[:, 0].tolist() == [1.0, 2.0, -1.0] and len({tuple(q) + tuple(b) for q, b in zip(qv, boost)}) == 3
    for order in A.BIG_ORDERS:
        W, L = A.big_world(order, metric), E.big_world(order)
        assert W.n_docs == L.n_docs and W.dels == L.dels
        assert all(np.array_equal(a[1], b[1]) for a, b in zip(W.stores, L.stores))     # E.BIG_DOCS' layout
        assert _all_bf16(W, qv, boost) and W.n_live_vectors() > 4000
        assert _exact_in_f32(W, qv, metric) < 2.0 ** 20
        # the order, as queries 0 and 2 (boost -1) see it
        _, _, lists = A.big_lists(order, metric)
        for q in (0, 2):
            sc, sg, dc = lists[q][0]
            d = np.diff(sc[np.argsort(sg * E.BIG_DOCS[0] + dc)].astype(F64))
            if order == "tied":
                assert np.all(d == 0)
            else:
                assert np.all(d > 0) if (order == "asc") != (q == 2) else np.all(d < 0)


@pytest.mark.parametrize("metric", A.BIG_METRICS)
def test_big_world_moves_under_its_mutations(metric):
    """a stage's rows taken from the previous tile (top-k form, 4 tiles per workgroup) and tile_begin taken as 0
    (store form): each moves the output of some case, and the model without a mutation is the reference"""
    total = sum(E.BIG_DOCS)
    qv, boost = A.big_queries(metric)
    moved = {"prev_tile_rows": 0, "tile_begin_zero": 0}
    for order in A.BIG_ORDERS:
        W = A.big_world(order, metric)
        _model_is_the_reference(W, qv, boost, metric, 65)
        for R in A.BIG_TOPK:
            tpb = A.topk_grid(total, 3, R, 256)[1]
            moved["prev_tile_rows"] += _moves(W, qv, boost, metric, R, "prev_tile_rows", tpb=tpb)
        for _, R in A.BIG_STORE:
            n = _moves(W, qv, boost, metric, R, "tile_begin_zero", chunk_docs=E.store_steps(total, R)[0])
            moved["tile_begin_zero"] += n
            if order == "asc":      # the best docs of queries 0 and 1 lie in the last step
                assert n >= 2
    assert moved["prev_tile_rows"] > 0 and moved["tile_begin_zero"] > 0


def test_dim_worlds():
    assert {A.stages(d) for d in A.DIMS} == {1, 2, 3, 4, 5, 16}
    for edge in (64, 128, 192, 256):
        assert {edge - 1, edge, edge + 1} <= set(A.DIMS) or {edge, edge + 1} <= set(A.DIMS)
        assert A.stages(edge) + 1 == A.stages(edge + 1)
    assert sum(1 for d in A.DIMS if d % 4) >= 10 and max(A.DIMS) == 1024
    for dim in A.DIMS:
        # the two-clause call and the shifted device pointer take the scalar query loads; dims % 4 == 0 otherwise not
        assert A.qvec4(A.SMALL_DIM + dim, A.SMALL_DIM) == 0 and A.qvec4(dim, 0, ptr=4) == 0
        assert A.qvec4(dim, 0) == (dim % 4 == 0)
        for metric in (0, 1):
            W, qv, boost, small = A.dim_world(dim, metric)
            assert 290 <= W.total <= 310 and (W.stores[1] is None) == (dim % 2 == 1) and len(W.n_docs) in (2, 3)
            assert _all_bf16(W, qv, boost) and all(A.is_bf16(st[2]) for st in small)
            assert all(st[2].shape[1] == A.SMALL_DIM for st in small)
            for st in W.stores:
                if st is not None:
                    assert np.all(np.abs(st[2][:, -1]) == 0.5) and (dim == 1 or np.abs(st[2][:, :-1]).max() <= 7 / 16)
                    assert len(set(st[2][:, -1].tolist())) == 2
            if dim > 1:
                assert np.all(np.abs(qv[:, -1]) == 0.5) and np.abs(qv[:, :-1]).max() <= 7 / 16
            assert _exact_in_f32(W, qv, metric) * 256 < 2.0 ** 19      # integers / 256
            assert all(W.n_live_vectors() > c for c in A.DIM_CANDS)
            for R in A.DIM_CANDS:
                _model_is_the_reference(W, qv, boost, metric, R)
                assert _moves(W, qv, boost, metric, R, "drop_last_dim") > 0, (dim, metric, R)
                if dim > A.KC // 2:
                    assert _moves(W, qv, boost, metric, R, "drop_second_kstep") > 0, (dim, metric, R)


def test_query_tile_worlds():
    assert A.QUERY_TILE_NQS == (15, 16, 17, 63, 64, 65, 129)
    for metric in (0, 1):
        W = A.query_tile_world(metric)
        assert W.total == 300 and W.n_live_vectors() > 100
        moved = {"neighbour_query": 0, "unmasked_lanes": 0}
        for nq in A.QUERY_TILE_NQS:
            qv, boost = A.query_tile_queries(nq)
            assert len({tuple(q) for q in qv.tolist()}) == nq and len(set(boost[:, 0].tolist())) == nq
            assert np.all(boost != 0) and _all_bf16(W, qv, boost)
            assert _exact_in_f32(W, qv, metric) * 256 <= 2.0 ** 11
            if metric == 0:     # score * boost is exact: at most 10 + 8 significant bits
                assert np.abs(boost).max() * 64 < 2 ** 8 and np.all(boost * 64 == np.round(boost * 64))
            for R in A.QUERY_TILE_CANDS:
                if nq in (17, 129):
                    _model_is_the_reference(W, qv, boost, metric, R)
                for mut in moved:
                    moved[mut] += _moves(W, qv, boost, metric, R, mut)
        assert all(moved.values()), moved


def test_doc_tile_worlds():
    assert A.DOC_TILE_WORLDS == (1, 127, 128, 129, 256, 257, "3seg")
    qv, boost = A.doc_tile_queries()
    for metric in (0, 1):
        moved = 0
        for name in A.DOC_TILE_WORLDS:
            W = A.doc_tile_world(name, metric)
            assert _all_bf16(W, qv, boost) and _exact_in_f32(W, qv, metric) * 256 <= 2.0 ** 11
            if name == "3seg":
                assert np.cumsum(W.n_docs).tolist() == [64, 128, 129] and W.stores[1] is None
                assert W.stores[2][1][0] != E.NOVEC and W.n_live_vectors() < 70
            else:
                assert W.n_docs == [name] and E.n_tiles(name) == (name + 127) // 128
                assert W.stores[0][1][0] != E.NOVEC and W.stores[0][1][-1] != E.NOVEC
            for R in A.DOC_TILE_CANDS:
                _model_is_the_reference(W, qv, boost, metric, R)
                moved += _moves(W, qv, boost, metric, R, "drop_row_127")
        assert A.doc_tile_world(127, metric).n_live_vectors() > 70 > E.SMALL_K
        assert moved > 0


def test_nan_world():
    W = E.nan_world()
    qv, boost = A.nan_queries()
    assert _all_bf16(W, qv, boost) and len(set(qv[:, 0].tolist())) == 4
    assert not A.is_bf16(E.exact_queries(4, 8)[0])          # why this file has queries of its own
    rows, ok = A.flat_view(W)
    fin = np.where(np.isinf(rows), 0, rows)
    assert np.isinf(rows[list(E.NAN_FLATS), 3]).all() and np.all(qv[:, 3] == 0)
    for q in qv:        # the finite products are exact: one nonzero term per row
        assert np.count_nonzero(fin * q[None, :], axis=1).max() == 1
        assert np.array_equal((fin[:, 0] * q[0]).astype(F64), fin[:, 0].astype(F64) * float(q[0]))
    n = len([f for f in E.NAN_FLATS + E.ZERO_FLATS if W.live(0, f // 80, f % 80)])
    assert 4 < n < 64 < W.n_live_vectors() <= 160
    assert sum(_moves(W, qv, boost, 0, R, "keep_nan") for R in (4, n, 64, 160)) > 0


@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("dim", A.GENERAL_DIMS)
def test_general_bands(dim, metric):
    """the seeds keep the band condition: per query and R at most max(2, R // 10) docs besides the R-th are free"""
    assert A.GENERAL_R == (20, 64, 100) and [A.general_band_limit(R) for R in A.GENERAL_R] == [2, 6, 10]
    assert E.BUF_CAP_NARROW > 20 <= E.SMALL_K // 2 < 64 <= E.SMALL_K < 100      # narrow cap, wide cap, store form
    assert A.stages(dim) >= 2 and dim % 4 == 1 or dim == 1024
    W, qv, boost = A.general_world(dim, metric)
    assert W.total == 600 and len(W.n_docs) == 2 and len(qv) == 8 and W.n_live_vectors() > 500
    assert not A.is_bf16(qv) and not A.is_bf16(W.stores[0][2])
    for keys, m, delta in A.general_model(W, qv, boost, metric):
        assert len(keys) == W.n_live_vectors() and np.all(delta > 0) and np.all(np.isfinite(delta))
        for R in A.GENERAL_R:
            t, must, never, band = A.general_band(m, delta, R)
            assert int(band.sum()) - 1 <= A.general_band_limit(R)
            assert must.sum() + never.sum() + band.sum() == len(m) and R - band.sum() <= must.sum() < R
            # the check has teeth: the band is narrow against the spread of the scores it cuts
            assert (delta + delta.max()).max() < 0.05 * (m.max() - m.min())


def test_model_bound_covers_f32_summation_orders():
    """the delta of the model covers what plain f32 accumulation of the bf16 products gives in three orders
    (left to right, right to left, blocks of 32 then left to right), with room: the device's order is a fourth"""
    for dim, metric in ((257, 0), (1024, 1)):
        W, qv, boost = A.general_world(dim, metric)
        rows, ok = A.flat_view(W)
        X = A.bf16_round(rows[ok])
        for q in range(3):
            qb = A.bf16_round(qv[q])
            m, delta = A.first_pass_model(rows[ok], qv[q], boost[q, 0], metric)
            P = np.zeros((len(X), A.dim_pad(dim)), F32)
            P[:, :dim] = X * qb[None, :]
            blocks = P.reshape(len(X), -1, 32).astype(F32)
            sums = (np.cumsum(P, axis=1, dtype=F32)[:, -1], np.cumsum(P[:, ::-1], axis=1, dtype=F32)[:, -1],
                    np.cumsum(np.cumsum(blocks, axis=2, dtype=F32)[:, :, -1], axis=1, dtype=F32)[:, -1])
            for s in sums:
                if metric == 0:
                    dev = (s * boost[q, 0]).astype(F32)
                else:
                    nrm, qn = A.norms_l2r(rows[ok]), A.norms_l2r(qv[q][None, :])[0]
                    D = ((nrm + qn).astype(F32) - (F32(2.0) * s).astype(F32)).astype(F32)
                    dev = ((-np.sqrt(np.maximum(D, F32(0.0)))).astype(F32) * boost[q, 0]).astype(F32)
                assert np.all(np.abs(dev.astype(F64) - m) <= delta)
