"""Hybrid text + vector search on the device (slg_batch_prepare_hybrid, slg_batch_hybrid_device,
slg_search_batch_hybrid) through the C ABI against tests/hybrid_ref.py.  BM25 parts are bit-exact; a clause
similarity and the final score agree within 1e-5, the summed vector score within 1e-5 x n_clauses; exact ties
come out in (segment, doc) order; a query is left out of the order check only when the reference's own gap at
a clause's cand_size boundary or at the k_out boundary is below 4e-5, and at most 10 % of a case's queries.  Of
such a query the rows the near-tie cannot move (docs outside hybrid_ref's `near` set) are still compared."""
import numpy as np
import pytest

from tests import hybrid_ref as R
from tests.util import random_queries, random_segment, _append_lists

pytestmark = pytest.mark.gpu
TOL = 1e-5
GAP = 4e-5
F32 = np.float32
NOVEC = 0xFFFFFFFF


def _unit(rng, n, dim):
    v = rng.standard_normal((n, dim)).astype(F32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True).astype(F32)).astype(F32)


def _store(rng, n_docs, dim, metric, p_missing=0.2):
    have = rng.random(n_docs) >= p_missing
    rows = int(have.sum())
    offs = np.full(n_docs, NOVEC, np.uint32)
    offs[np.nonzero(have)[0]] = rng.permutation(rows)
    vals = _unit(rng, max(rows, 1), dim) if metric == 0 else rng.standard_normal((max(rows, 1), dim)).astype(F32)
    return metric, offs, vals


def _world(rng, n_docs, vocab, dim, metric, p_missing=0.2, avg_len=6):
    """segments with text and a vector store in field 0 -> (segs, field 0's stores)"""
    segs, stores = [], []
    for n in n_docs:
        s = random_segment(rng, n, vocab, avg_len)
        st = _store(rng, n, dim, metric, p_missing)
        s.vec_dim, s.vec_metric, s.vec_offsets, s.vec_values = dim, metric, st[1], st[2]
        segs.append(s)
        stores.append(st)
    return segs, stores


def _qvecs(rng, nq, dims, metrics):
    return np.concatenate([_unit(rng, nq, d) if m == 0 else rng.standard_normal((nq, d)).astype(F32)
                           for d, m in zip(dims, metrics)], axis=1)


def _close(a, b, tol=TOL):
    return a == b or abs(float(a) - float(b)) <= tol


def check(got, want, k_out, nc, metric0, what):
    doc, seg, score, vec, count, total = got
    skipped = 0
    for q, w in enumerate(want):
        print(f"{what} q{q}: total {int(total[q])} / {w['total']}, count {int(count[q])}, gap {w['gap']:.3g}")
        rows = w["rows"]
        if w["gap"] < GAP:  # no order, total or count check; a row the near-tie cannot move keeps its scores
            skipped += 1
            assert int(count[q]) <= k_out
            wmap = {(r[0], r[1]): r for r in rows}
            for i in range(int(count[q])):
                key = (int(seg[q, i]), int(doc[q, i]))
                if key in wmap and key not in w["near"]:
                    wv = R.missing(metric0) if wmap[key][3] is None else wmap[key][3]
                    assert _close(score[q, i], wmap[key][2]), f"{what} q{q} row {i}: score (near-tie query)"
                    assert _close(vec[q, i], wv, TOL * nc), f"{what} q{q} row {i}: vec (near-tie query)"
            continue
        assert int(total[q]) == w["total"], f"{what} q{q}: total {total[q]} != {w['total']}"
        n = min(k_out, w["total"])
        assert int(count[q]) == n, f"{what} q{q}: count {count[q]} != {n}"
        wmap = {(r[0], r[1]): r for r in rows}
        for i in range(n):
            assert _close(score[q, i], rows[i][2]), f"{what} q{q} row {i}: score {score[q, i]} != {rows[i][2]}"
            key = (int(seg[q, i]), int(doc[q, i]))
            if key != (rows[i][0], rows[i][1]):  # only a near-tie may swap; an exact tie may not
                assert key in wmap and rows[i][2] != wmap[key][2] and _close(wmap[key][2], rows[i][2], 2 * TOL), \
                    f"{what} q{q} row {i}: {key} != {rows[i][:2]}"
            if key in wmap:
                wv = wmap[key][3]
                wv = R.missing(metric0) if wv is None else wv  # None: the missing score of clause 0's metric
                assert _close(vec[q, i], wv, TOL * nc), f"{what} q{q} row {i}: vec {vec[q, i]} != {wv}"
        assert np.all(doc[q, n:] == 0) and np.all(score[q, n:] == 0)
    share = skipped / max(len(want), 1)
    print(f"{what}: {skipped} of {len(want)} queries left out of the order check")
    assert share <= 0.10, f"{what}: {share:.0%} of the queries have a boundary gap below {GAP}"


def _case(oracle, ix, segs, fields, clause_field, qs, k, qv, alpha, boost, cand, k_out, what, q_filter=None,
          filters=None, **plans):
    got = ix.search_hybrid(*qs, k, clause_field, qv, alpha, cand, k_out, boost=boost, q_filter=q_filter, **plans)
    want = R.reference(oracle, segs, fields, clause_field, *qs, k, qv, alpha, boost, cand, k_out,
                       q_filter=q_filter, filters=filters, **plans)
    metric0 = next(st[0] for st in fields[clause_field[0]] if st is not None)
    check(got, want, k_out, len(clause_field), metric0, what)
    return got, want


@pytest.mark.parametrize("nc,metric,multi", [(1, 0, False), (1, 1, False), (2, 0, True), (2, 1, False),
                                             (8, 0, True)])
def test_clauses_fields_metrics(oracle, nc, metric, multi):
    """1, 2 and 8 clauses over one and several fields, cosine and L2, docs without vectors, three segments,
    tombstones"""
    import searchlite_amd as sa
    rng = np.random.default_rng(100 * nc + metric)
    n_docs, vocab, dim = [400, 333, 150], 40, 24
    segs, st0 = _world(rng, n_docs, vocab, dim, metric)
    segs[0].set_deleted([1, 5, 77, 399])
    segs[2].set_deleted(range(0, 150, 7))
    st1 = [_store(rng, n_docs[0], 10, 1), None, _store(rng, n_docs[2], 10, 1, p_missing=0.5)]
    st2 = [None, _store(rng, n_docs[1], 768, 0), _store(rng, n_docs[2], 768, 0)]
    fields = [st0, st1, st2]
    clause_field = [(c % 3) if multi else 0 for c in range(nc)]
    dims = [[dim, 10, 768][f] for f in clause_field]
    metrics = [[metric, 1, 0][f] for f in clause_field]
    nq = 12
    qs = random_queries(rng, nq, 3, vocab, n_segs=3, weights=True)
    qv = _qvecs(rng, nq, dims, metrics)
    alpha = rng.choice(np.array([0.0, 0.3, 0.5, 0.8, 1.0], F32), size=(nq, nc)).astype(F32)
    boost = (rng.random((nq, nc)) + 0.5).astype(F32)
    with sa.GpuIndex(segs) as ix:
        assert ix.add_vector_field(st1) == 1 and ix.add_vector_field(st2) == 2
        _case(oracle, ix, segs, fields, clause_field, qs, 11, qv, alpha, boost, 20, 11, f"nc{nc} m{metric}")
        _case(oracle, ix, segs, fields, clause_field, qs, 11, qv, 0.0, None, 20, 11, f"nc{nc} m{metric} vec-only")


def test_filter_and_score_plan(oracle):
    """q_filter, and a DisMax plan over leaves of two terms (the multi-field query-string shape) through the
    prepared, device-chained form"""
    import searchlite_amd as sa
    rng = np.random.default_rng(7)
    n_docs, vocab, dim = [500, 300], 30, 16
    segs, st0 = _world(rng, n_docs, vocab, dim, 0)
    segs[1].set_deleted([0, 2, 4])
    nq = 10
    qs = random_queries(rng, nq, 4, vocab, n_segs=2)
    qv = _qvecs(rng, nq, [dim], [0])
    masks = [rng.random(n) < 0.6 for n in n_docs]
    q_filter = np.array([0 if q % 2 == 0 else -1 for q in range(nq)], np.int32)
    plans = dict(q_leaf=np.tile(np.array([0, 0, 1, 1], np.uint32), nq), q_plan=np.full(nq, 1, np.int32),
                 q_tie=np.full(nq, 0.3, F32), q_nleaves=np.full(nq, 2, np.uint32))
    with sa.GpuIndex(segs) as ix:
        assert ix.add_filter(masks) == 0
        _case(oracle, ix, segs, [st0], [0], qs, 11, qv, 0.4, None, 15, 11, "filter", q_filter=q_filter,
              filters=[masks])
        _case(oracle, ix, segs, [st0], [0], qs, 11, qv, 0.4, None, 15, 11, "filter+plan", q_filter=q_filter,
              filters=[masks], **plans)


def test_nothing_and_everything(oracle):
    import searchlite_amd as sa
    from searchlite_amd.segment import NO_TERM
    rng = np.random.default_rng(11)
    n_docs, vocab, dim = [300, 200], 20, 8
    segs, st0 = _world(rng, n_docs, vocab, dim, 0)
    segs = [_append_lists(s, [(np.arange(s.n_docs, dtype=np.uint32), np.ones(s.n_docs, np.uint32))]) for s in segs]
    for s, st in zip(segs, st0):
        s.vec_dim, s.vec_metric, s.vec_offsets, s.vec_values = dim, 0, st[1], st[2]
    offs = np.array([0, 1, 2, 3, 5], np.uint32)
    terms = np.array([[NO_TERM, NO_TERM], [vocab, vocab], [3, 3], [vocab, vocab], [5, NO_TERM]], np.uint32)
    w = np.ones(5, F32)
    qv = _qvecs(rng, 4, [dim], [0])
    with sa.GpuIndex(segs) as ix:
        got, want = _case(oracle, ix, segs, [st0], [0], (offs, terms, w), 11, qv, 0.5, None, 50, 11, "none/all")
    assert int(got[5][0]) == 0 and int(got[4][0]) == 0           # the query that matches nothing
    assert want[1]["total"] == 11 + 50 - len(set(h[:2] for h in want[1]["bm25"]) & set(want[1]["maps"][0]))


@pytest.mark.parametrize("cand", [1, 64, 65, 7000])
def test_cand_sizes(oracle, cand):
    """cand_size 1, 64, 65, and 7000: with 12 000 matched docs, 9 600 of them with a vector, the fold takes more
    than one pass (a boost of 40 spreads the 9 600 scores: the reference's own gap at rank 7000 stays above 4e-5)"""
    import searchlite_amd as sa
    rng = np.random.default_rng(cand)
    n_docs = [12000] if cand == 7000 else [700, 500]
    vocab, dim = 30, 8
    segs, st0 = _world(rng, n_docs, vocab, dim, 0, avg_len=4)
    segs = [_append_lists(s, [(np.arange(s.n_docs, dtype=np.uint32), np.ones(s.n_docs, np.uint32))]) for s in segs]
    for s, st in zip(segs, st0):
        s.vec_dim, s.vec_metric, s.vec_offsets, s.vec_values = dim, 0, st[1], st[2]
    nq = 10
    offs, terms, w = random_queries(rng, nq, 2, vocab, n_segs=len(n_docs))
    terms[0::2] = vocab  # every query's first term: the list that holds every doc
    qv = _qvecs(rng, nq, [dim], [0])
    with sa.GpuIndex(segs) as ix:
        boost = np.full((nq, 1), 40.0 if cand == 7000 else 1.0, F32)
        _case(oracle, ix, segs, [st0], [0], (offs, terms, w), 11, qv, 0.3, boost, cand, 11, f"cand {cand}")


@pytest.mark.parametrize("k,k_out", [(1, 1), (11, 11), (1001, 1001), (0, 11)])
def test_k_and_k_out(oracle, k, k_out):
    """k = 0: no BM25 hits, the union is the clause lists alone (bm25 = 0.0 everywhere)"""
    import searchlite_amd as sa
    rng = np.random.default_rng(k + 50)
    n_docs, vocab, dim = [1500, 900], 25, 12
    segs, st0 = _world(rng, n_docs, vocab, dim, 0)
    nq = 10
    qs = random_queries(rng, nq, 3, vocab, n_segs=2)
    qv = _qvecs(rng, nq, [dim], [0])
    with sa.GpuIndex(segs) as ix:
        _case(oracle, ix, segs, [st0], [0], qs, k, qv, 0.5, None, 100, k_out, f"k {k}")


def _all_docs_world(rng, n_docs, vocab, dim):
    """_world plus a term (id = vocab) that every doc holds"""
    segs, st0 = _world(rng, n_docs, vocab, dim, 0, avg_len=4)
    segs = [_append_lists(s, [(np.arange(s.n_docs, dtype=np.uint32), np.ones(s.n_docs, np.uint32))]) for s in segs]
    for s, st in zip(segs, st0):
        s.vec_dim, s.vec_metric, s.vec_offsets, s.vec_values = dim, 0, st[1], st[2]
    return segs, st0


@pytest.mark.parametrize("nc,cand,k,n_docs", [(8, 1000, 1001, [1500, 1200]), (3, 7000, 11, [12000])])
def test_union_and_bm25_sort_space_in_global_memory(oracle, nc, cand, k, n_docs):
    """vs_blend_kernel<true>'s work space outside LDS.  8 clauses x 1000 + k 1001: the union keys (16384) fill
    LDS and the BM25 hits sort in global memory; 3 clauses x 7000: the union keys (32768) sort in global memory
    too.  (A boost of 40 spreads the scores: the reference's own boundary gaps stay above 4e-5.)"""
    import searchlite_amd as sa
    rng = np.random.default_rng(1000 * nc + 1)
    vocab, dim = 30, 8
    segs, st0 = _all_docs_world(rng, n_docs, vocab, dim)
    nq = 10
    offs, terms, w = random_queries(rng, nq, 2, vocab, n_segs=len(n_docs))
    terms[0::2] = vocab
    qv = _qvecs(rng, nq, [dim] * nc, [0] * nc)
    alpha = rng.choice(np.array([0.0, 0.3, 0.6], F32), size=(nq, nc)).astype(F32)
    boost = np.full((nq, nc), 40.0, F32)
    with sa.GpuIndex(segs) as ix:
        _case(oracle, ix, segs, [st0], [0] * nc, (offs, terms, w), k, qv, alpha, boost, cand, 11, f"nc{nc} cand{cand}")


def test_key_area_that_does_not_fit_is_oom_and_leaves_the_batch_usable(oracle):
    """pool_cap_mb 4 -> 1 MiB of keys; with 8 clauses that is 16384 candidate slots, and a query over the
    all-docs list of 20000 docs has more: SLG_ERR_OOM before any launch.  The same batch then serves a call
    that fits (one clause), with the right result: nothing was launched or half-written."""
    import searchlite_amd as sa
    from searchlite_amd import _native as N
    rng = np.random.default_rng(404)
    vocab, dim = 20, 8
    segs, st0 = _all_docs_world(rng, [20000], vocab, dim)
    nq = 3
    offs, terms, w = random_queries(rng, nq, 2, vocab, n_segs=1)
    terms[0::2] = vocab
    qv8 = _qvecs(rng, nq, [dim] * 8, [0] * 8)
    qv1 = np.ascontiguousarray(qv8[:, :dim])
    boost = np.full((nq, 1), 40.0, F32)
    with sa.GpuIndex(segs, tuning={"pool_cap_mb": 4}) as ix:
        with ix.prepare(offs, terms, w, 11, hybrid=True) as b:
            with pytest.raises(N.SlgError) as ei:
                b.hybrid([0] * 8, qv8, 0.5, 50, 11)
            assert ei.value.code == N.ERR_OOM and "key work area" in ei.value.msg
            got = b.hybrid([0], qv1, 0.5, 50, 11, boost=boost)
    want = R.reference(oracle, segs, [st0], [0], offs, terms, w, 11, qv1, 0.5, boost, 50, 11)
    check(got, want, 11, 1, 0, "after OOM")


def test_sharded_runs_refuse_a_hybrid_batch(oracle):
    import searchlite_amd as sa
    from searchlite_amd import searcher, _native as N
    rng = np.random.default_rng(6)
    segs, _ = _world(rng, [300], 10, 8, 0)
    qs = random_queries(rng, 2, 2, 10)
    with sa.GpuIndex(segs) as ix:
        group = searcher.ShardGroup(ix, 0, 1, searcher.shard_unique_id(), 1)
        with ix.prepare(*qs, 11, hybrid=True) as b:
            for call in (lambda: b.run_sharded(group), lambda: b.run_sharded(group, fetch=False),
                         lambda: b.run_sharded(group, fetch=False, seq=0), b.fetch_sharded):
                with pytest.raises(N.SlgError) as ei:
                    call()
                assert ei.value.code == N.ERR_UNSUPPORTED
            b.run()  # the batch itself is untouched
            assert int(b.fetch()[3].sum()) > 0
        group.close()


def test_device_chained_equals_host_form_and_rows_equal_plans(oracle):
    import searchlite_amd as sa
    rng = np.random.default_rng(21)
    n_docs, vocab, dim = [800, 600], 30, 32
    segs, st0 = _world(rng, n_docs, vocab, dim, 1)
    segs[0].set_deleted(range(3, 800, 11))
    nq = 16
    qs = random_queries(rng, nq, 3, vocab, n_segs=2, weights=True)
    qv = _qvecs(rng, nq, [dim, dim], [1, 1])
    alpha = np.tile(np.array([[0.25, 0.0]], F32), (nq, 1))
    with sa.GpuIndex(segs) as ix:
        host = ix.search_hybrid(*qs, 11, [0, 0], qv, alpha, 30, 11)
        with ix.prepare(*qs, 11, hybrid=True) as b:
            dev = b.hybrid([0, 0], qv, alpha, 30, 11)
            rows = b.fetch()
            again = b.hybrid([0, 0], qv, alpha, 30, 11)  # a second call on the same batch
        with ix.prepare(*qs, 11) as p:
            p.run()
            plain = p.fetch()
    for a, b_, c in zip(host, dev, again):
        assert np.array_equal(a.view(np.uint8), b_.view(np.uint8)) and np.array_equal(a.view(np.uint8), c.view(np.uint8))
    for a, b_ in zip(rows[:4], plain[:4]):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b_).view(np.uint8))
    want = oracle.search_batch(segs, *qs, 11)
    assert np.array_equal(rows[2].view(np.uint32), want[2].view(np.uint32)) and np.array_equal(rows[0], want[0])


def test_after_update_deleted_and_key_ranges(oracle):
    """after slg_index_update_deleted; and with a small buffer pool the queries go through in several ranges"""
    import searchlite_amd as sa
    rng = np.random.default_rng(33)
    n_docs, vocab, dim = [9000, 7000], 12, 8
    segs, st0 = _world(rng, n_docs, vocab, dim, 0, avg_len=5)
    nq = 10
    qs = random_queries(rng, nq, 3, vocab, n_segs=2)
    qv = _qvecs(rng, nq, [dim], [0])
    with sa.GpuIndex(segs, tuning={"pool_cap_mb": 4, "updatable": 1}) as ix:
        with ix.prepare(*qs, 11, hybrid=True) as b:  # 1 MiB of keys: the batch's slots do not fit one range
            slots = sum(int(s.term_offsets[t + 1] - s.term_offsets[t]) for i, s in enumerate(segs)
                        for t in qs[1][:, i])
            assert slots * 8 > (1 << 20)
        _case(oracle, ix, segs, [st0], [0], qs, 11, qv, 0.5, None, 40, 11, "ranges")
        segs[1].set_deleted(range(0, 7000, 3))
        ix.update_deleted(1, segs[1].deleted, float(segs[1].docs))
        _case(oracle, ix, segs, [st0], [0], qs, 11, qv, 0.5, None, 40, 11, "after update")


def test_error_codes(oracle):
    import searchlite_amd as sa
    from searchlite_amd import _native as N
    rng = np.random.default_rng(5)
    segs, st0 = _world(rng, [200], 10, 8, 0)
    qs = random_queries(rng, 2, 2, 10)
    qv = _qvecs(rng, 2, [8], [0])

    def code(f):
        with pytest.raises(N.SlgError) as ei:
            f()
        return ei.value.code

    with sa.GpuIndex(segs) as ix:
        assert code(lambda: ix.search_hybrid(*qs, 11, [0] * 9, np.tile(qv, (1, 9)), 0.5, 10, 11)) == N.ERR_UNSUPPORTED
        assert code(lambda: ix.search_hybrid(*qs, 11, [], qv, np.zeros((2, 0), F32), 10, 11)) == N.ERR_UNSUPPORTED
        assert code(lambda: ix.search_hybrid(*qs, 11, [0], qv, 0.5, 0, 11)) == N.ERR_UNSUPPORTED
        assert code(lambda: ix.search_hybrid(*qs, 11, [0], qv, 0.5, N.MAX_VECTOR_CANDIDATES + 1, 11)) == N.ERR_UNSUPPORTED
        assert code(lambda: ix.search_hybrid(*qs, N.MAX_K + 1, [0], qv, 0.5, 10, 11)) == N.ERR_UNSUPPORTED
        assert code(lambda: ix.search_hybrid(*qs, 11, [0], qv, 0.5, 10, N.MAX_K + 1)) == N.ERR_UNSUPPORTED
        assert code(lambda: ix.search_hybrid(*qs, 11, [3], qv, 0.5, 10, 11)) == N.ERR_INVALID  # no such field
        lib = ix._lib
        with ix.prepare(*qs, 11) as p:  # not a hybrid batch
            p.run()
            assert code(lambda: p.hybrid_device([0], 1, 1, None, 10, 11, 1, 1, 1, 1, 1, 1)) == N.ERR_INVALID
        with ix.prepare(*qs, 11, hybrid=True) as b:
            assert code(lambda: b.hybrid_device([0], 1, 1, None, 10, 11, 1, 1, 1, 1, 1, 1)) == N.ERR_INVALID  # not run
            b.run()
            assert code(lambda: b.hybrid_device([0], None, 1, None, 10, 11, 1, 1, 1, 1, 1, 1)) == N.ERR_INVALID
            assert code(lambda: b.hybrid_device([0], 1, 1, None, 10, 11, None, 1, 1, 1, 1, 1)) == N.ERR_INVALID
            assert code(b.matched_counts) == N.ERR_UNSUPPORTED
            assert code(b.cursor_seen) == N.ERR_UNSUPPORTED
            assert lib.slg_batch_fetch_sharded(b._h, None, None, None, None) == N.ERR_UNSUPPORTED


def test_vector_only_search_is_unchanged(oracle):
    """slg_vector_search_batch on one fixed case (both cand_size paths) against the numpy reference of
    tests/test_gpu_vector_search.py: vs_select_kernel and vs_blend_kernel are shared with the hybrid search"""
    import searchlite_amd as sa
    from tests import test_gpu_vector_search as V
    rng = np.random.default_rng(2024)
    dim = 24
    stores = [V._store(rng, 700, dim, 0), V._store(rng, 500, dim, 0)]
    segs = [V._seg(700, *stores[0][1:]), V._seg(500, *stores[1][1:])]
    for cand in (20, 200):
        nq = 4
        boost = np.ones((nq, 1), F32)
        qv = V._queries(oracle, rng, [stores], [0], [dim], nq, boost, cand, [0])
        with sa.GpuIndex(segs) as ix:
            got = ix.vector_search([0], qv, 0.0, cand, 11)
        want = V.reference(oracle, [stores], [0], [0], qv, np.zeros((nq, 1), F32), boost, cand, 11)
        V.check(got, want, 11, f"vector-only cand {cand}")
