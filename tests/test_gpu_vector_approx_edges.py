"""vs_scan_bf16_kernel (slg_vsearch_approx.hpp), the first pass of the two-pass vector search, at its structural
edges: several tiles per workgroup, chunk steps of the store form (tile_begin > 0), the 64-dimension staging step
and its prefetch chain up to 16 stages deep, scalar query loads (a clause offset that is no multiple of 4, an
unaligned device pointer), query and doc tiles that are not full, cosine NaN -> 0, and on general data the docs the
first pass picks against a float64 model of what it computes.

The worlds are tests/vector_approx_edge_worlds.py (A); tests/test_vector_approx_edge_worlds.py proves on the CPU
that each reaches the path its case names, that every value in the exact worlds is a bf16 value and every score
exact in f32 in any order, and that a named defect of the first pass would move the output of its family.

Exact worlds: the first pass computes the exact scan's scores there, so the two-pass call must return the exact
call's bytes (`same`) at refine = cand, where nothing but the first pass decides the list.  The same rows must be
the host reference's bit for bit and in order (`exact`), which keeps the exact call from vouching for itself.

General data, cand = refine = k_out = R: the returned docs are the first pass's best R.  A doc whose model score
lies above the model's R-th by more than the error bound of A.first_pass_model must be returned, one as far below
must not be; the docs in between are free (A's docstring derives the bound; the CPU file holds the free docs per
query to max(2, R // 10)).

Not asserted: L2 over non-finite values, for the reason at the top of tests/test_gpu_vector_edges.py.  A segment
whose field has another dimension than the rest cannot reach the scan (field_facts refuses the call:
test_a_segment_of_another_dimension_is_refused), so the kernel's dim_pad comparison is not reachable from a test.
"""
import numpy as np
import pytest

from tests import test_gpu_vector_search as V
from tests import vector_approx_edge_worlds as A
from tests import vector_edge_worlds as E
from tests.test_gpu_vector_approx import same
from tests.test_gpu_vector_edges import exact

pytestmark = pytest.mark.gpu
F32 = np.float32


def _zeros(nq, nc=1):
    return np.zeros((nq, nc), F32)


def both(ix, clause_field, qv, cand, refine, k_out, boost, want, what):
    """the two-pass call against the exact call (bytes) and against the reference (bits, order)"""
    ex = ix.vector_search(clause_field, qv, 0.0, cand, k_out, boost=boost)
    got = ix.vector_search_approx(clause_field, qv, 0.0, cand, refine, k_out, boost=boost)
    same(got, ex, what)
    exact(got, want, k_out, what)
    return got


def _want(W, metric, qv, boost, cand, k_out):
    lists = E.sorted_lists([W.stores], [0], qv, boost, W.live_masks)
    return E.reference_from_lists(lists, [metric], [0], _zeros(len(qv)), cand, k_out)


@pytest.fixture(scope="module")
def big_index():
    """one quantised index per (order, metric) of the 98 049-doc world, built on first use, kept for the module"""
    import searchlite_amd as sa
    held = {}

    def get(order, metric):
        if (order, metric) not in held:
            ix = sa.GpuIndex(A.big_world(order, metric).segs())
            ix.quantize_vector_field(0)
            held[order, metric] = ix
        return held[order, metric]
    yield get
    for ix in held.values():
        ix.close()


@pytest.mark.parametrize("metric", A.BIG_METRICS)
@pytest.mark.parametrize("order", A.BIG_ORDERS)
@pytest.mark.parametrize("cand", A.BIG_TOPK)
def test_multi_tile_blocks(big_index, order, metric, cand):
    """767 tiles over at most 255 workgroups per query tile: at least 4 tiles per workgroup, so the threshold, the
    buffer and s_seg / s_doc / s_nrm are carried over tiles and drow is recomputed after a prefetch chain; the last
    tile holds one doc, the segment boundary lies inside a tile.  cand 32 / 33: both buffer caps."""
    qv, boost, lists = A.big_lists(order, metric)
    want = E.reference_from_lists(lists, [metric], [0], _zeros(3), cand, cand)
    got = both(big_index(order, metric), [0], qv, cand, cand, cand, boost, want,
               f"multi-tile {order} metric {metric} cand {cand}")
    assert np.all(got[5] == cand) and np.all(got[4] == cand)


@pytest.mark.parametrize("metric", A.BIG_METRICS)
@pytest.mark.parametrize("order", A.BIG_ORDERS)
@pytest.mark.parametrize("cand,refine", A.BIG_STORE)
def test_store_form_steps(big_index, order, metric, cand, refine):
    """refine > 64: 7 chunk steps (refine 65) and 8 (refine 4000), tile_begin > 0 from the second on.  Ascending:
    the best docs lie in the last step; descending with refine > cand: a wrong tile_begin offset would return docs
    of the first step only, which the negative boost of query 2 turns into the worst"""
    qv, boost, lists = A.big_lists(order, metric)
    k_out = min(cand, 1001)
    want = E.reference_from_lists(lists, [metric], [0], _zeros(3), cand, k_out)
    got = both(big_index(order, metric), [0], qv, cand, refine, k_out, boost, want,
               f"store {order} metric {metric} cand {cand} refine {refine}")
    assert np.all(got[5] == cand)


def _device_outs(ix, nq, ptr, da, db, cand, k_out):
    import torch
    dev = torch.device("cuda", 0)
    od = torch.zeros((nq, k_out), dtype=torch.int32, device=dev)
    os_, osc, ov = torch.zeros_like(od), torch.zeros((nq, k_out), device=dev), torch.zeros((nq, k_out), device=dev)
    oc = torch.zeros(nq, dtype=torch.int32, device=dev)
    ot = torch.zeros(nq, dtype=torch.int64, device=dev)
    ix.vector_search_approx_device(nq, [0], ptr, da.data_ptr(), db.data_ptr(), None, cand, cand, k_out,
                                   od.data_ptr(), os_.data_ptr(), osc.data_ptr(), ov.data_ptr(), oc.data_ptr(),
                                   ot.data_ptr())
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (od, os_, osc, ov, oc, ot)]


@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("dim", A.DIMS)
def test_dim_steps(metric, dim):
    """dims on both sides of the 64-dimension staging step up to a prefetch chain of 16 stages; the last component
    of every row and query is the largest, so a dropped, doubled or misplaced tail crosses many ranks.  Three ways
    in: alone (16-byte query loads when dim % 4 == 0), as the second clause behind a 3-dimension field (scalar
    query loads: qvec4 == 0), and through the device form with the queries 4 bytes past a 16-byte boundary (the
    shifted buffer holds one float more than the queries, so every address read lies inside it)."""
    import torch
    import searchlite_amd as sa
    W, qv, boost, small = A.dim_world(dim, metric)
    nq = len(qv)
    rng = np.random.default_rng(dim)
    q2 = np.concatenate([A._grid(rng, (nq, A.SMALL_DIM)), qv], axis=1)
    boost2 = np.concatenate([boost[::-1], boost], axis=1)
    fields, metrics, cf = [W.stores, small], [metric, 0], [1, 0]
    lists2 = E.sorted_lists(fields, cf, q2, boost2, W.live_masks)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    aligned = t(qv)
    shifted = torch.zeros(nq * dim + 1, dtype=torch.float32, device=dev)
    shifted[1:] = aligned.reshape(-1)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 0
    da, db = t(_zeros(nq)), t(boost)
    with sa.GpuIndex(W.segs()) as ix:
        assert ix.add_vector_field(small) == 1
        ix.quantize_vector_field(0)
        ix.quantize_vector_field(1)
        for cand in A.DIM_CANDS:
            what = f"metric {metric} dim {dim} cand {cand}"
            got = both(ix, [0], qv, cand, cand, cand, boost, _want(W, metric, qv, boost, cand, cand), what)
            both(ix, cf, q2, cand, cand, 2 * cand, boost2,
                 E.reference_from_lists(lists2, metrics, cf, _zeros(nq, 2), cand, 2 * cand), what + ", second clause")
            outs = [_device_outs(ix, nq, ptr, da, db, cand, cand) for ptr in (aligned.data_ptr(), shifted.data_ptr() + 4)]
            same(outs[1], outs[0], what + ", unaligned device pointer")
            same(outs[0], got, what + ", device form")


@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("cand", A.QUERY_TILE_CANDS)
@pytest.mark.parametrize("nq", A.QUERY_TILE_NQS)
def test_query_tile_edges(nq, cand, metric):
    """query counts around 16 (a wave) and 64 (a tile), and 129 = two tiles + one query: pairwise distinct queries
    and boosts, every query checked, so a query row staged from another or a lane past nq shows"""
    import searchlite_amd as sa
    W = A.query_tile_world(metric)
    qv, boost = A.query_tile_queries(nq)
    with sa.GpuIndex(W.segs()) as ix:
        ix.quantize_vector_field(0)
        both(ix, [0], qv, cand, cand, 12, boost, _want(W, metric, qv, boost, cand, 12),
             f"nq {nq} cand {cand} metric {metric}")


@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("cand", A.DOC_TILE_CANDS)
@pytest.mark.parametrize("world", A.DOC_TILE_WORLDS)
def test_doc_tile_edges(world, cand, metric):
    """1, 127, 128, 129, 256 and 257 docs in one segment; segments of 64, 64 and 1 docs whose middle one lacks the
    field"""
    import searchlite_amd as sa
    W = A.doc_tile_world(world, metric)
    qv, boost = A.doc_tile_queries()
    with sa.GpuIndex(W.segs()) as ix:
        ix.quantize_vector_field(0)
        got = both(ix, [0], qv, cand, cand, 71, boost, _want(W, metric, qv, boost, cand, 71),
                   f"docs {world} cand {cand} metric {metric}")
    assert np.all(got[5] == min(cand, W.n_live_vectors()))


def test_a_segment_of_another_dimension_is_refused():
    """segments that disagree on the field's dimension: the copies are built (each with its own dim_pad), and both
    searches refuse the call before any scan, so no row of a copy of another dim_pad is ever read"""
    import searchlite_amd as sa
    from searchlite_amd import _native as N
    rng = np.random.default_rng(5)
    a, b = A.grid_store(rng, 100, 8, 0), A.grid_store(rng, 60, 72, 0)
    assert A.dim_pad(8) != A.dim_pad(72)
    with sa.GpuIndex([V._seg(100, a[1], a[2]), V._seg(60, b[1], b[2])]) as ix:
        ix.quantize_vector_field(0)
        assert ix.fetch_vector_copy(0, 0, 8)[0].shape[1] == 8 and ix.fetch_vector_copy(0, 1, 72)[0].shape[1] == 72
        qv = A._grid(rng, (2, 8))
        for call in (lambda: ix.vector_search([0], qv, 0.0, 5, 5), lambda: ix.vector_search_approx([0], qv, 0.0, 5, 5, 5)):
            with pytest.raises(N.SlgError) as e:
                call()
            assert e.value.code == N.ERR_INVALID and "vec_dim" in str(e.value)


def test_cosine_nan_is_zero_in_the_first_pass():
    """rows with inf (a bf16 value) where the query holds 0.0: the first pass's sum is NaN and its score 0.0 * boost,
    so these rows rank among the zero vectors by (segment, doc), in the first pass as in the exact scan"""
    import searchlite_amd as sa
    W = E.nan_world()
    qv, boost = A.nan_queries()
    flats = sorted(f for f in E.NAN_FLATS + E.ZERO_FLATS if W.live(0, f // 80, f % 80))
    with sa.GpuIndex(W.segs()) as ix:
        ix.quantize_vector_field(0)
        for cand in (4, len(flats), 64, 160):
            got = both(ix, [0], qv, cand, cand, 160, boost, _want(W, 0, qv, boost, cand, 160), f"nan cand {cand}")
            n = min(cand, len(flats))
            assert [(int(got[1][0, i]), int(got[0][0, i])) for i in range(n)] == [(f // 80, f % 80) for f in flats[:n]]
            assert np.all(got[2][0, :n] == 0) and np.all(got[2][0, n:min(cand, int(got[5][0]))] < 0)


@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("dim", A.GENERAL_DIMS)
def test_general_data_first_pass_picks_the_models_docs(dim, metric):
    """random vectors, cand = refine = k_out = R in {20, 64, 100} (narrow cap, wide cap, store form): the returned
    docs are the first pass's best R.  Against the float64 model of the bf16 products: every doc above the model's
    R-th score by more than the error bound is there, none as far below it is, and every returned score is the exact
    call's for that doc."""
    import searchlite_amd as sa
    W, qv, boost = A.general_world(dim, metric)
    model = A.general_model(W, qv, boost, metric)
    n_all = W.total
    with sa.GpuIndex(W.segs()) as ix:
        ix.quantize_vector_field(0)
        edoc, eseg, esc, evec, ecnt, _ = ix.vector_search([0], qv, 0.0, n_all, n_all, boost=boost)
        outs = {R: ix.vector_search_approx([0], qv, 0.0, R, R, R, boost=boost) for R in A.GENERAL_R}
    for q, (keys, m, delta) in enumerate(model):
        ex = {(int(eseg[q, i]), int(edoc[q, i])): (esc[q, i].tobytes(), evec[q, i].tobytes()) for i in range(int(ecnt[q]))}
        assert set(ex) == set(keys)
        for R in A.GENERAL_R:
            doc, seg, sc, vec, cnt, tot = outs[R]
            what = f"dim {dim} metric {metric} R {R} q{q}"
            assert int(cnt[q]) == R and int(tot[q]) == R, what
            rows = [(int(seg[q, i]), int(doc[q, i])) for i in range(R)]
            assert len(set(rows)) == R, what
            for i, key in enumerate(rows):
                assert ex[key] == (sc[q, i].tobytes(), vec[q, i].tobytes()), f"{what} row {i}: not the exact score"
            t, must, never, band = A.general_band(m, delta, R)
            back = set(rows)
            lost = [keys[i] for i in np.nonzero(must)[0] if keys[i] not in back]
            wrong = [keys[i] for i in np.nonzero(never)[0] if keys[i] in back]
            print(f"{what}: t {t:.6g} max delta {delta.max():.3g} band {int(band.sum()) - 1} lost {lost} wrong {wrong}")
            assert not lost, f"{what}: docs above the band are missing: {lost}"
            assert not wrong, f"{what}: docs below the band were returned: {wrong}"
