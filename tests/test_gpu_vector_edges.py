"""vs_scan_kernel, vs_select_kernel and vs_blend_kernel<false> (slg_vsearch.hpp) at their structural edges: several
tiles per workgroup, query tiles and waves that are not full, doc tiles and segment boundaries, the 32-dimension
staging step, an unaligned device query pointer, the union's sort space in global memory, chunk steps of the store
path under adversarial order, and the score-value edges of the key encoding.

The worlds are tests/vector_edge_worlds.py; tests/test_vector_edge_worlds.py proves on the CPU that each holds what
its case here relies on (tile, block, chunk-step and sort-space counts from the kernels' constants) and that the
vectorised reference used for the 98 049-doc world equals the oracle-backed one of tests/test_gpu_vector_search.py.

Exact-score worlds: rows (v, 0, .., 0) against queries (x, 0, .., 0): the matrix cores' fma chain and the oracle's
left-to-right sum both give round(v * x), so scores are compared bit for bit (`exact`) and the order has to be the
reference's at every row (exact_order=True).  Nothing is skipped there.  Random-vector cases keep TOL and the gap
rule of test_gpu_vector_search.

Not asserted: L2 over non-finite values.  (a - b)^2 sums to NaN there, and the sign of that NaN is
platform-defined (x86 produces a negative one, the GPU a positive one); f32::total_cmp ranks the two at opposite
ends, so the reference on the host and the device would disagree with both following the same arithmetic.
"""
import numpy as np
import pytest

from tests import test_gpu_vector_search as V
from tests import vector_edge_worlds as E

pytestmark = pytest.mark.gpu
F32 = np.float32


def exact(got, want, k_out, what):
    """V.check with exact order, and every score and vector score bit-identical to the reference's"""
    V.check(got, want, k_out, what, exact_order=True)
    doc, seg, score, vec, count, total = got
    for q, (rows, tot, _) in enumerate(want):
        n = min(k_out, tot)
        ws = np.array([r[2] for r in rows[:n]], F32)
        wv = np.array([r[3] for r in rows[:n]], F32)
        assert np.array_equal(score[q, :n].view(np.uint32), ws.view(np.uint32)), f"{what} q{q}: score bits"
        assert np.array_equal(vec[q, :n].view(np.uint32), wv.view(np.uint32)), f"{what} q{q}: vec bits"


def _zeros(nq, nc=1):
    return np.zeros((nq, nc), F32)


@pytest.fixture(scope="module")
def big_index():
    """one index per order of the 98 049-doc world, built on first use and kept for the module"""
    import searchlite_amd as sa
    held = {}

    def get(order):
        if order not in held:
            W = E.big_random_world() if order == "random" else E.big_world(order)
            held[order] = sa.GpuIndex(W.segs())
        return held[order]
    yield get
    for ix in held.values():
        ix.close()


@pytest.mark.parametrize("order", E.BIG_ORDERS)
@pytest.mark.parametrize("cand", [1, 32, 33, 64])
def test_multi_tile_blocks(big_index, order, cand):
    """767 tiles over at most 255 workgroups per query tile: every workgroup but the last takes >= 4 tiles, the last
    fewer, the final tile holds one doc, and the segment boundary lies inside a tile.  Ascending scores make every
    doc beat the threshold carried from tile to tile (the buffer folds in mid-scan, over and over), descending
    scores make every later tile fail the ballot, ties leave (segment, doc) to decide.  Query 2 has boost -1:
    it sees the reverse order."""
    qv, boost, lists = E.big_lists(order)
    got = V._run(big_index(order), [0], qv, 0.0, cand, cand, boost=boost)
    want = E.reference_from_lists(lists, [0], [0], _zeros(3), cand, cand)
    exact(got, want, cand, f"multi-tile {order} cand {cand}")
    assert np.all(got[5] == cand) and np.all(got[4] == cand)


@pytest.mark.parametrize("cand", [32, 64])
def test_multi_tile_blocks_random_vectors(big_index, cand):
    """the same layout with random unit vectors: the non-exact path over several tiles per workgroup (TOL, and
    queries whose boundary gap is >= 1e-4)"""
    qv, boost, lists = E.big_random_lists()
    got = V._run(big_index("random"), [0], qv, 0.0, cand, cand + 1, boost=boost)
    want = E.reference_from_lists(lists, [0], [0], _zeros(3), cand, cand + 1)
    V.check(got, want, cand + 1, f"multi-tile random cand {cand}")


@pytest.mark.parametrize("order", E.BIG_ORDERS)
@pytest.mark.parametrize("cand", [65, 4000])
def test_store_path_steps(big_index, order, cand):
    """cand_size > 64: 7 chunk steps of 16 256 docs (cand 65), 8 of 12 288 (cand 4000).  Ascending: every step
    replaces the whole running list; descending: `key > th` rejects every later step; tied: (segment, doc)."""
    qv, boost, lists = E.big_lists(order)
    k_out = min(cand, 1001)
    got = V._run(big_index(order), [0], qv, 0.0, cand, k_out, boost=boost)
    want = E.reference_from_lists(lists, [0], [0], _zeros(3), cand, k_out)
    exact(got, want, k_out, f"store {order} cand {cand}")
    assert np.all(got[5] == cand)


@pytest.mark.parametrize("cand", [8, 100])
@pytest.mark.parametrize("nq", E.QUERY_TILE_NQS)
def test_query_tile_edges(oracle, nq, cand):
    """query counts around 16 (a wave) and 64 (a tile), and 129 = two tiles + one query: pairwise distinct queries
    and boosts, every query checked bit for bit, so a row staged from another query or a lane past nq shows"""
    import searchlite_amd as sa
    W = E.query_tile_world()
    qv, boost = E.exact_queries(nq, 8)
    with sa.GpuIndex(W.segs()) as ix:
        got = V._run(ix, [0], qv, 0.0, cand, 12, boost=boost)
    want = V.reference(oracle, [W.stores], [0], [0], qv, _zeros(nq), boost, cand, 12, W.live)
    exact(got, want, 12, f"nq {nq} cand {cand}")


@pytest.mark.parametrize("cand", [5, 70])
@pytest.mark.parametrize("world", E.DOC_TILE_TOTALS + ("3seg",))
def test_doc_tile_edges(oracle, world, cand):
    """1, 127, 128, 129, 256 and 257 docs in one segment; and segments of 64, 64 and 1 docs (boundaries at flats 64,
    128 and 129) whose middle one lacks the field"""
    import searchlite_amd as sa
    W = E.doc_tile_world(world)
    qv, boost = E.exact_queries(3, 8)
    with sa.GpuIndex(W.segs()) as ix:
        got = V._run(ix, [0], qv, 0.0, cand, 71, boost=boost)
    want = V.reference(oracle, [W.stores], [0], [0], qv, _zeros(3), boost, cand, 71, W.live)
    exact(got, want, 71, f"docs {world} cand {cand}")
    assert np.all(got[5] == min(cand, W.n_live_vectors()))


@pytest.mark.parametrize("metric,dim", [(m, d) for m in (0, 1) for d in E.DIM_STEPS[m]])
def test_dim_steps(oracle, metric, dim):
    """dimensions on both sides of the 32-dimension staging step (36: a vec4 row that ends 4 floats into the second
    step) and L2 at dimensions that are no multiple of 4 (vs_ld4's scalar branch); the last component of every row
    and query is large (E.DIM_TAIL), so a dropped or doubled tail moves every score by 1e4 x TOL"""
    import searchlite_amd as sa
    W, qv, boost = E.dim_world(dim, metric)
    nq = len(qv)
    with sa.GpuIndex(W.segs()) as ix:
        for cand in (20, 70):
            got = V._run(ix, [0], qv, 0.0, cand, 11)
            want = V.reference(oracle, [W.stores], [metric], [0], qv, _zeros(nq), boost, cand, 11, W.live)
            V.check(got, want, 11, f"metric {metric} dim {dim} cand {cand}")


def test_unaligned_device_query_pointer():
    """the device form with qvecs 4 bytes past a 16-byte boundary: dim 64 keeps the rows' 16-byte loads (vec4) while
    the queries take the scalar loads (qvec4 == 0).  The outputs are byte-identical to the aligned call.  The
    shifted buffer holds one float more than the queries, so every address read lies inside it."""
    import torch
    import searchlite_amd as sa
    rng = np.random.default_rng(19)
    dim, nq = 64, 21
    stores = [V._store(rng, 400, dim, 0), V._store(rng, 310, dim, 0)]
    segs = [V._seg(400, *stores[0][1:]), V._seg(310, *stores[1][1:])]
    qv = V._unit(rng, nq, dim)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    aligned = t(qv)
    base = torch.zeros(nq * dim + 1, dtype=torch.float32, device=dev)
    base[1:] = aligned.reshape(-1)
    assert aligned.data_ptr() % 16 == 0 and base.data_ptr() % 16 == 0
    da, db = t(np.full((nq, 1), 0.25, F32)), t(np.full((nq, 1), 1.5, F32))
    with sa.GpuIndex(segs) as ix:
        for cand, k_out in ((20, 11), (300, 301)):
            outs = []
            for ptr in (aligned.data_ptr(), base.data_ptr() + 4):
                od = torch.zeros((nq, k_out), dtype=torch.int32, device=dev)
                os_, osc, ov = torch.zeros_like(od), torch.zeros((nq, k_out), device=dev), torch.zeros((nq, k_out), device=dev)
                oc = torch.zeros(nq, dtype=torch.int32, device=dev)
                ot = torch.zeros(nq, dtype=torch.int64, device=dev)
                ix.vector_search_device(nq, [0], ptr, da.data_ptr(), db.data_ptr(), None, cand, k_out, od.data_ptr(),
                                        os_.data_ptr(), osc.data_ptr(), ov.data_ptr(), oc.data_ptr(), ot.data_ptr())
                torch.cuda.synchronize()
                outs.append([x.cpu().numpy() for x in (od, os_, osc, ov, oc, ot)])
            assert np.all(outs[0][4] == min(k_out, cand)) and np.all(outs[0][5] == cand)
            for a, b in zip(*outs):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"cand {cand}"


@pytest.mark.parametrize("k_out", [11, 1001])
@pytest.mark.parametrize("nc,cand", E.UNION_CASES)
def test_union_in_global_memory(nc, cand, k_out):
    """vs_blend_kernel<false> with P = 32 768 > kVsSortCap: 2 clauses x 9000 and 3 x 5500 (an odd clause count) over
    two fields; boost 40 spreads the scores and the queries keep a boundary gap >= 1e-4.  The summed vector score is
    held to TOL x n_clauses, the rule of the hybrid twin (test_gpu_hybrid): under boost 40 a clause score lies near
    20 .. 40, where f32 values are 1.9e-6 .. 3.8e-6 apart, and the sum of n_clauses of them takes a rounding of that
    size per clause, on the device as in the reference.  The final score keeps TOL."""
    import searchlite_amd as sa
    W, fields, clause_field, qv, alpha, boost, lists = E.union_world(nc, cand)
    segs = W.segs()
    with sa.GpuIndex(segs) as ix:
        assert ix.add_vector_field(fields[1]) == 1
        got = V._run(ix, clause_field, qv, alpha, cand, k_out, boost=boost)
    metrics = [0, 0]
    want = E.reference_from_lists(lists, metrics, clause_field, alpha, cand, k_out)
    V.check(got, want, k_out, f"union nc{nc} cand{cand} k_out{k_out}", vec_tol=V.TOL * nc)
    for q, (_, tot, maps) in enumerate(want):
        assert int(got[5][q]) == tot == len(set().union(*[m.keys() for m in maps])) and tot > cand


def test_negative_boost_and_signed_zero(oracle):
    """boost -1 reverses the order; zero vectors score +0.0 and -0.0 after the multiply.  Clause 0 (boost -1) over
    field 0 and clause 1 (boost +1) over an all-zero field: with alpha 0 a doc's final is (c0 + c1) / 2, and the
    order among -0.0 (a zero row of field 0 found by both lists), +0.0 and the negatives is f32::total_cmp's."""
    import searchlite_amd as sa
    A, B, zeros = E.signed_zero_world()
    fields = [A.stores, B.stores]
    with sa.GpuIndex(A.segs()) as ix:
        assert ix.add_vector_field(B.stores) == 1
        _signed_zero_cases(oracle, ix, A, fields, zeros)


def _signed_zero_cases(oracle, ix, A, fields, zeros):
    for nc, cf in ((1, [0]), (2, [0, 1])):
        nq = 4
        qv = np.zeros((nq, 8 * nc), F32)
        qv[:, 0] = (1.0 + np.arange(nq) / 256.0).astype(F32)
        boost = np.ones((nq, nc), F32)
        boost[:, 0] = [-1.0, -2.0, -1.0, 1.0]
        if nc == 2:
            qv[:, 8] = 1.0
        for cand in (6, 10, 15, 70):   # inside the ten -0.0 rows, exactly them, past them; the store path
            got = V._run(ix, cf, qv, 0.0, cand, 80, boost=boost)
            want = V.reference(oracle, fields, [0, 0], cf, qv, _zeros(nq, nc), boost, cand, 80, A.live)
            exact(got, want, 80, f"signed zero nc{nc} cand {cand}")
            if nc == 1:  # the -0.0 rows lead queries 0..2 in (segment, doc) order, above every negative score
                live_zeros = [f for f in zeros if A.live(0, f // 60, f % 60)]
                n = min(cand, len(live_zeros))
                assert [(int(got[1][0, i]), int(got[0][0, i])) for i in range(n)] == [(f // 60, f % 60) for f in live_zeros[:n]]
                # (the blend starts its sums at +0.0, so the final and the vector score of a -0.0 clause score are +0.0)
                assert np.all(got[2][0, :n].view(np.uint32) == 0) and np.all(got[2][0, n:cand] < 0)
                assert np.all(got[2][3, :cand] > 0)


def test_cosine_nan_is_zero(oracle):
    """rows with inf where the query holds 0.0: the sum is NaN, the score 0.0 * boost, and they rank among the real
    zeros (zero vectors) by (segment, doc): under boost -1 both kinds are -0.0 in the clause list, above every negative
    score, under boost +1 they are +0.0 below every positive one"""
    import searchlite_amd as sa
    W = E.nan_world()
    qv, _ = E.exact_queries(4, 8)
    boost = np.array([[-1.0], [1.0], [-2.0], [2.0]], F32)
    flats = sorted(f for f in E.NAN_FLATS + E.ZERO_FLATS if W.live(0, f // 80, f % 80))
    with sa.GpuIndex(W.segs()) as ix:
        for cand in (4, len(flats), 64, 160):
            got = V._run(ix, [0], qv, 0.0, cand, 160, boost=boost)
            want = V.reference(oracle, [W.stores], [0], [0], qv, _zeros(4), boost, cand, 160, W.live)
            exact(got, want, 160, f"nan cand {cand}")
            n = min(cand, len(flats))
            assert [(int(got[1][0, i]), int(got[0][0, i])) for i in range(n)] == [(f // 80, f % 80) for f in flats[:n]]
            assert np.all(got[2][0, :n] == 0) and np.all(got[2][0, n:min(cand, int(got[5][0]))] < 0)
    # with every live vector in the list the zeros close query 1's rows, +0.0
    tot = int(got[5][1])
    assert tot == W.n_live_vectors()
    assert np.all(got[2][1, tot - len(flats):tot].view(np.uint32) == 0)
