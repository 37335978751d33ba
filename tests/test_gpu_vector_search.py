"""Exact vector-only search on the device (slg_vector_search_batch*) against a numpy restatement of
search_vector_only (api/reader.rs:2187-2330) with collect_vector_maps' per-segment HNSW search
replaced by an exact scan and the filter applied before the truncation.  Per-segment similarities
come from the C oracle (oracle.rerank at alpha 0: a left-to-right f32 sum); the boost is an f32
multiply (api/reader.rs:2421); merging, truncation, union and blend are restated here.  The cosine
scan runs on the f32 matrix cores (an fmaf chain), so scores agree to 1e-5 and orders are checked
away from near-ties; exact ties must come out in (segment, doc) order exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-5
NOVEC = 0xFFFFFFFF
F32 = np.float32


def _seg(n_docs, offsets=None, values=None, metric=0):
    from searchlite_amd.segment import Segment
    kw = {}
    if values is not None:
        kw = dict(vec_dim=values.shape[1], vec_metric=metric, vec_offsets=np.asarray(offsets, np.uint32),
                  vec_values=np.ascontiguousarray(values, np.float32))
    return Segment(n_docs=n_docs, term_offsets=[0, 1], doc_ids=[0], tfs=[1],
                   field_doc_len=[np.ones(n_docs, np.float32)], field_avgdl=[1.0], docs=float(n_docs), **kw)


def _unit(rng, n, dim):
    v = rng.standard_normal((n, dim)).astype(F32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True).astype(F32)).astype(F32)


def _store(rng, n_docs, dim, metric, p_missing=0.2, values=None):
    """(metric, offsets, values) of one segment: some docs without a vector, rows out of doc order."""
    have = rng.random(n_docs) >= p_missing
    rows = int(have.sum())
    perm = rng.permutation(rows)
    offs = np.full(n_docs, NOVEC, np.uint32)
    offs[np.nonzero(have)[0]] = perm
    if values is None:
        values = _unit(rng, rows, dim) if metric == 0 else rng.standard_normal((rows, dim)).astype(F32)
    return metric, offs, values[:rows]


def _tkey(x):
    b = np.array(x, F32).view(np.int32).astype(np.int64)
    return int(b ^ ((b >> 31) & 0x7FFFFFFF))


def _clause_scores(oracle, field, qv, bst, live):
    """[(score, seg, doc)] of every live doc with a vector in the field, sorted as collect_vector_maps."""
    ents = []
    for s, st in enumerate(field):
        if st is None:
            continue
        metric, offs, vals = st
        docs = np.array([d for d in range(len(offs)) if offs[d] != NOVEC and live(s, d)], np.uint32)
        if len(docs) == 0:
            continue
        od, _, ov = oracle.rerank(metric, offs, vals, qv, 0.0, docs, np.zeros(len(docs), F32), len(docs))
        for d, v in zip(od, ov):
            ents.append((F32(v) * F32(bst), s, int(d)))
    ents.sort(key=lambda e: (-_tkey(e[0]), e[1], e[2]))
    return ents


def blend_rows(maps, metrics, clause_field, alpha_q, k_out):
    """the union of one query's clause lists ({(seg, doc): score} each), compute_hybrid_score at bm25 = 0, sorted:
    (rows [(seg, doc, final, vec)] of the top k_out, the union size)"""
    nc = len(maps)
    old = np.seterr(over="ignore", invalid="ignore")
    union = set().union(*[m.keys() for m in maps])
    rows = []
    for key in union:
        bsum, vsum = F32(0.0), F32(0.0)
        for c in range(nc):
            if key in maps[c]:
                vs = maps[c][key]
                vsum = F32(vsum + vs)
            else:
                vs = F32(-1.0) if metrics[clause_field[c]] == 0 else F32(np.finfo(F32).min)
            a = F32(alpha_q[c])
            if a >= 1:
                bl = F32(0.0)
            elif a <= 0:
                bl = vs
            else:
                bl = F32(F32(a * F32(0.0)) + F32(F32(F32(1.0) - a) * vs))
            bsum = F32(bsum + bl)
        rows.append((key[0], key[1], F32(bsum / F32(nc)), vsum))
    rows.sort(key=lambda r: (-_tkey(r[2]), r[0], r[1]))
    np.seterr(**old)
    return rows[:k_out], len(union)


def reference(oracle, fields, metrics, clause_field, qvecs, alpha, boost, cand, k_out, live=None):
    """Per query: rows [(seg, doc, final, vec)] of the top k_out, the union size, the clause lists."""
    nq, nc = alpha.shape
    dims = [next(st[2].shape[1] for st in fields[f] if st is not None) for f in clause_field]
    offs = np.concatenate([[0], np.cumsum(dims)])
    old = np.seterr(over="ignore", invalid="ignore")
    out = []
    for q in range(nq):
        lv = (lambda s, d: True) if live is None else (lambda s, d, q=q: live(q, s, d))
        maps = []
        for c, f in enumerate(clause_field):
            ents = _clause_scores(oracle, fields[f], qvecs[q, offs[c]:offs[c + 1]], boost[q, c], lv)[:cand]
            maps.append({(s, d): v for v, s, d in ents})
        rows, total = blend_rows(maps, metrics, clause_field, alpha[q], k_out)
        out.append((rows, total, maps))
    np.seterr(**old)
    return out


def boundary_gap(oracle, fields, clause_field, qv_parts, bst, cand, live=None):
    """smallest score gap at a clause's cand_size boundary (inf when the list is not truncated)"""
    gap = np.inf
    for c, f in enumerate(clause_field):
        if bst[c] == 0:  # every score is +-0: the order is (segment, doc) on both sides
            continue
        ents = _clause_scores(oracle, fields[f], qv_parts[c], bst[c], live or (lambda s, d: True))
        if len(ents) > cand:
            gap = min(gap, abs(float(ents[cand - 1][0]) - float(ents[cand][0])))
    return gap


def _close(a, b, tol=TOL):
    return a == b or abs(float(a) - float(b)) <= tol


def check(got, want, k_out, what, exact_order=False, vec_tol=TOL):
    """vec_tol: the bound on the summed vector score (TOL unless a caller states why its sums need more)"""
    doc, seg, score, vec, count, total = got
    for q, (rows, tot, _) in enumerate(want):
        assert int(total[q]) == tot, f"{what} q{q}: total {total[q]} != {tot}"
        n = min(k_out, tot)
        assert int(count[q]) == n, f"{what} q{q}: count"
        wmap = {(r[0], r[1]): r for r in rows}
        for i in range(n):
            assert _close(score[q, i], rows[i][2]), f"{what} q{q} row {i}: score {score[q, i]} != {rows[i][2]}"
            key = (int(seg[q, i]), int(doc[q, i]))
            if exact_order:
                assert key == (rows[i][0], rows[i][1]), f"{what} q{q} row {i}: {key} != {rows[i][:2]}"
            elif key != (rows[i][0], rows[i][1]):
                assert key in wmap and _close(wmap[key][2], rows[i][2], 2 * TOL), f"{what} q{q} row {i}: order"
            if key in wmap:
                assert _close(vec[q, i], wmap[key][3], vec_tol), f"{what} q{q} row {i}: vec {vec[q, i]} != {wmap[key][3]}"
        assert np.all(doc[q, n:] == 0) and np.all(score[q, n:] == 0)


def _queries(oracle, rng, fields, clause_field, dims, nq, boost, cand, metric_of, live=None):
    """queries whose clause-boundary gaps are >= 1e-4 (redrawn otherwise)"""
    qs = []
    while len(qs) < nq:
        parts = [(_unit(rng, 1, d)[0] if metric_of[c] == 0 else rng.standard_normal(d).astype(F32))
                 for c, d in enumerate(dims)]
        if boundary_gap(oracle, fields, clause_field, parts, boost[len(qs)], cand, live) >= 1e-4:
            qs.append(np.concatenate(parts))
    return np.stack(qs).astype(F32)


def _run(ix, clause_field, qvecs, alpha, cand, k_out, boost=None, q_filter=None):
    return ix.vector_search(clause_field, qvecs, alpha, cand, k_out, boost=boost, q_filter=q_filter)


@pytest.mark.parametrize("dim", [1, 6, 100, 768, 1030])
def test_dims_cosine(oracle, dim):
    import searchlite_amd as sa
    rng = np.random.default_rng(dim)
    stores = [_store(rng, 300, dim, 0), _store(rng, 257, dim, 0), None, _store(rng, 90, dim, 0)]
    segs = [_seg(300, *stores[0][1:]), _seg(257, *stores[1][1:]), _seg(40), _seg(90, *stores[3][1:])]
    segs[0].set_deleted([3, 7, 100, 299])
    segs[3].set_deleted(range(0, 90, 5))
    dels = {0: {3, 7, 100, 299}, 3: set(range(0, 90, 5))}
    live = lambda q, s, d: d not in dels.get(s, ())
    cand = 1 if dim == 1 else 20
    nq = 6
    boost = np.ones((nq, 1), F32)
    qv = _queries(oracle, rng, [stores], [0], [dim], nq, boost, cand, [0], lambda s, d: live(0, s, d)) if dim > 1 else \
        np.array([[1.0], [-1.0], [0.5], [1.0], [-0.25], [2.0]], F32)
    with sa.GpuIndex(segs) as ix:
        got = _run(ix, [0], qv, 0.0, cand, 11)
    want = reference(oracle, [stores], [0], [0], qv, np.zeros((nq, 1), F32), boost, cand, 11, live)
    check(got, want, 11, f"dim {dim}", exact_order=dim == 1)


# the epilogue's widths (32: the narrow buffer, 64 = kVsSmallK) and + 1 (65: the chunked path),
# the chunked path, 10000, and a cand_size above the number of live vectors
@pytest.mark.parametrize("cand", [1, 2, 32, 33, 63, 64, 65, 128, 1000, 10000])
def test_cand_size_boundaries(oracle, cand):
    import searchlite_amd as sa
    rng = np.random.default_rng(cand)
    dim = 24
    n0, n1 = (700, 500) if cand < 10000 else (6000, 5000)
    stores = [_store(rng, n0, dim, 0), _store(rng, n1, dim, 0)]
    segs = [_seg(n0, *stores[0][1:]), _seg(n1, *stores[1][1:])]
    nq = 4
    boost = np.ones((nq, 1), F32)
    qv = _queries(oracle, rng, [stores], [0], [dim], nq, boost, cand, [0])
    k_out = min(cand + 1, 1001)
    with sa.GpuIndex(segs) as ix:
        got = _run(ix, [0], qv, 0.0, cand, k_out)
    want = reference(oracle, [stores], [0], [0], qv, np.zeros((nq, 1), F32), boost, cand, k_out)
    check(got, want, k_out, f"cand {cand}")


@pytest.mark.parametrize("cand,k_out", [(5, 4), (64, 10), (100, 7)])
def test_exact_ties_straddle_boundaries(oracle, cand, k_out):
    """duplicated vectors inside and across segments score bit-identically: (segment, doc) decides"""
    import searchlite_amd as sa
    rng = np.random.default_rng(cand)
    dim = 16
    base = _unit(rng, 1, dim)[0]
    stores, segs = [], []
    for s, n in enumerate((200, 150, 120)):
        m, offs, vals = _store(rng, n, dim, 0, p_missing=0.1)
        vals = vals.copy()
        dup = rng.choice(len(vals), size=min(len(vals), cand // 2 + 3), replace=False)
        vals[dup] = base  # the best score of the query, tied many times
        stores.append((m, offs, vals))
        segs.append(_seg(n, offs, vals))
    nq = 2
    qv = np.stack([base, base]).astype(F32)
    with sa.GpuIndex(segs) as ix:
        got = _run(ix, [0], qv, 0.0, cand, k_out)
    want = reference(oracle, [stores], [0], [0], qv, np.zeros((nq, 1), F32), np.ones((nq, 1), F32), cand, k_out)
    check(got, want, k_out, "ties", exact_order=True)
    # every clause-list member is a tied duplicate: the union is exactly the first cand (seg, doc) pairs
    assert int(got[5][0]) == cand


@pytest.mark.parametrize("cand", [10, 200])
def test_l2_near_duplicates(oracle, cand):
    import searchlite_amd as sa
    rng = np.random.default_rng(7 + cand)
    dim = 48
    m, offs, vals = _store(rng, 400, dim, 1)
    q = rng.standard_normal(dim).astype(F32)
    vals = vals.copy()
    eps = [0.0, 0.0, 1e-4, 2e-4, 5e-4, 1e-3, 3e-3, 1e-2]
    for i, e in enumerate(eps):  # near-duplicates of the query at distances down to ~1e-4, and copies
        d = rng.standard_normal(dim).astype(F32)
        vals[i] = (q + F32(e) * d / np.linalg.norm(d)).astype(F32)
    stores = [(1, offs, vals)]
    segs = [_seg(400, offs, vals, metric=1)]
    qv = q[None, :]
    with sa.GpuIndex(segs) as ix:
        got = _run(ix, [0], qv, 0.0, cand, 12)
    want = reference(oracle, [stores], [1], [0], qv, np.zeros((1, 1), F32), np.ones((1, 1), F32), cand, 12)
    check(got, want, 12, "l2 near-duplicates")
    assert got[2][0, 0] == 0.0 and got[2][0, 1] == 0.0  # exact copies: -sqrt(0) = -0.0, blended + 0 = 0


def _multi_index(rng, dims, metrics, n_docs=(260, 180)):
    """field 0 from the segment descriptors, fields 1.. through add_vector_field"""
    fields = []
    for f, (d, m) in enumerate(zip(dims, metrics)):
        fields.append([_store(rng, n, d, m, p_missing=0.3) for n in n_docs])
    fields[-1][1] = None if len(dims) > 1 else fields[-1][1]  # a segment without the last field
    return fields


@pytest.mark.parametrize("n_clauses", [2, 8])
def test_several_clauses_fields_metrics_alpha_boost(oracle, n_clauses):
    import searchlite_amd as sa
    rng = np.random.default_rng(100 + n_clauses)
    fdims, fmetrics = [32, 20, 7], [0, 1, 0]
    fields = _multi_index(rng, fdims, fmetrics)
    clause_field = [c % 3 for c in range(n_clauses)]
    dims = [fdims[f] for f in clause_field]
    nq, cand, k_out = 6, 12, 15
    boost = np.ones((nq, n_clauses), F32)
    boost[1, 0], boost[2, 1], boost[3, :] = 0.0, 2.0, 2.0
    qv = _queries(oracle, rng, fields, clause_field, dims, nq, boost, cand, [fmetrics[f] for f in clause_field])
    alpha = np.zeros((nq, n_clauses), F32)
    alpha[1] = 0.3
    alpha[2, 0] = 1.0
    alpha[4] = np.linspace(0.0, 1.0, n_clauses, dtype=F32)
    segs = [_seg(n, *fields[0][s][1:]) for s, n in enumerate((260, 180))]
    with sa.GpuIndex(segs) as ix:
        for f in (1, 2):
            assert ix.add_vector_field(fields[f]) == f
        got = _run(ix, clause_field, qv, alpha, cand, k_out, boost=boost)
    want = reference(oracle, fields, fmetrics, clause_field, qv, alpha, boost, cand, k_out)
    check(got, want, k_out, f"{n_clauses} clauses")
    # a doc outside one clause's list although it has a vector there takes the missing score
    rows, _, maps = want[0]
    assert any(key not in maps[1] and fields[clause_field[1]][key[0]] is not None and
               fields[clause_field[1]][key[0]][1][key[1]] != NOVEC for key in maps[0])
    # L2 clauses missing from f32::MIN sums: -inf finals exist when two L2 clauses miss a doc
    if n_clauses == 8:
        assert any(np.isneginf(r[2]) for q in want for r in q[0]) and np.isneginf(got[2][0]).any()


def test_filters_and_updates(oracle):
    import searchlite_amd as sa
    rng = np.random.default_rng(5)
    dim = 40
    stores = [_store(rng, 300, dim, 0), _store(rng, 200, dim, 0)]
    segs = [_seg(300, *stores[0][1:]), _seg(200, *stores[1][1:])]
    nq, cand, k_out = 4, 30, 31
    boost = np.ones((nq, 1), F32)
    qv = _queries(oracle, rng, [stores], [0], [dim], nq, boost, cand, [0])
    masks = [rng.random(300) < 0.5, rng.random(200) < 0.7]
    alpha = np.zeros((nq, 1), F32)
    with sa.GpuIndex(segs) as ix:
        fid = ix.add_filter(masks)
        q_filter = np.array([fid, -1, fid, -1], np.int32)
        dels = {}
        live = lambda q, s, d: d not in dels.get(s, ()) and (q_filter[q] < 0 or masks[s][d])
        got = _run(ix, [0], qv, alpha, cand, k_out, q_filter=q_filter)
        check(got, reference(oracle, [stores], [0], [0], qv, alpha, boost, cand, k_out, live), k_out, "filter")
        # tombstones: the next call follows the new state (the filter's bitmaps take them too)
        top = [int(got[1][q, 0]) * 1000 + int(got[0][q, 0]) for q in range(nq)]
        dels = {0: {t % 1000 for t in top if t < 1000} | {1, 2}, 1: {t % 1000 for t in top if t >= 1000}}
        for s, n in ((0, 300), (1, 200)):
            bits = np.zeros(n, bool)
            bits[list(dels[s])] = True
            ix.update_deleted(s, np.packbits(bits, bitorder="little"), float(n - bits.sum()))
        got = _run(ix, [0], qv, alpha, cand, k_out, q_filter=q_filter)
        check(got, reference(oracle, [stores], [0], [0], qv, alpha, boost, cand, k_out, live), k_out, "deleted")
        # a new segment (its docs come after the others')
        st2 = _store(rng, 150, dim, 0)
        assert ix.add_segment(_seg(150, *st2[1:])) == 2
        stores.append(st2)
        masks.append(np.ones(150, bool))
        got = _run(ix, [0], qv, alpha, cand, k_out)
        live2 = lambda q, s, d: d not in dels.get(s, ())
        check(got, reference(oracle, [stores], [0], [0], qv, alpha, boost, cand, k_out, live2), k_out, "added")


def test_device_form_is_bit_identical_to_host_form():
    import torch
    import searchlite_amd as sa
    rng = np.random.default_rng(9)
    dim = 64
    fields = [[_store(rng, 500, dim, 0), _store(rng, 300, dim, 0)], [_store(rng, 500, 12, 1), None]]
    segs = [_seg(500, *fields[0][0][1:]), _seg(300, *fields[0][1][1:])]
    nq, nc = 37, 2
    qv = np.concatenate([_unit(rng, nq, dim), rng.standard_normal((nq, 12)).astype(F32)], axis=1)
    alpha = np.full((nq, nc), 0.3, F32)
    boost = np.full((nq, nc), 1.5, F32)
    q_filter = np.where(np.arange(nq) % 3 == 0, 0, -1).astype(np.int32)
    with sa.GpuIndex(segs) as ix:
        assert ix.add_vector_field(fields[1]) == 1
        assert ix.add_filter([rng.random(500) < 0.5, None]) == 0
        for cand, k_out in ((20, 11), (300, 301)):
            want = _run(ix, [0, 1], qv, alpha, cand, k_out, boost=boost, q_filter=q_filter)
            dev = torch.device("cuda", 0)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            dq, da, db, df = t(qv), t(alpha), t(boost), t(q_filter)
            od = torch.zeros((nq, k_out), dtype=torch.int32, device=dev)
            os_, osc, ov = torch.zeros_like(od), torch.zeros((nq, k_out), device=dev), torch.zeros((nq, k_out), device=dev)
            oc = torch.zeros(nq, dtype=torch.int32, device=dev)
            ot = torch.zeros(nq, dtype=torch.int64, device=dev)
            ix.vector_search_device(nq, [0, 1], dq.data_ptr(), da.data_ptr(), db.data_ptr(), df.data_ptr(), cand, k_out,
                                    od.data_ptr(), os_.data_ptr(), osc.data_ptr(), ov.data_ptr(), oc.data_ptr(),
                                    ot.data_ptr())
            torch.cuda.synchronize()
            got = [x.cpu().numpy() for x in (od, os_, osc, ov, oc, ot)]
            for a, b in zip(got, want):
                assert np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_error_codes_then_a_valid_call(oracle):
    import searchlite_amd as sa
    from searchlite_amd import _native as N
    rng = np.random.default_rng(3)
    dim = 8
    stores = [_store(rng, 100, dim, 0)]
    segs = [_seg(100, *stores[0][1:])]
    qv = _unit(rng, 2, dim)
    lib = N.load()
    with sa.GpuIndex(segs) as ix:
        def rc(**kw):
            a = dict(cf=[0], q=qv, alpha=np.zeros((2, 1), F32), cand=5, k_out=3, q_filter=None)
            a.update(kw)
            try:
                _run(ix, a["cf"], a["q"], a["alpha"], a["cand"], a["k_out"], q_filter=a["q_filter"])
            except N.SlgError as e:
                return e.code
            return 0
        assert rc(cand=0) == N.ERR_UNSUPPORTED
        assert rc(cand=10001) == N.ERR_UNSUPPORTED
        assert rc(k_out=20002) == N.ERR_UNSUPPORTED
        assert rc(cf=[]) == N.ERR_UNSUPPORTED
        assert rc(cf=[0] * 9, q=np.tile(qv, 9), alpha=np.zeros((2, 9), F32)) == N.ERR_UNSUPPORTED
        assert rc(cf=[3]) == N.ERR_INVALID                      # no such vector field
        assert rc(q_filter=np.array([0, -1], np.int32)) == N.ERR_INVALID  # no such filter
        assert lib.slg_vector_search_batch(ix._h, 2, 1, np.zeros(1, np.uint32).ctypes.data, None, None, None, None,
                                           5, 3, None, None, None, None, None, None) == N.ERR_INVALID
        got = _run(ix, [0], qv, 0.0, 5, 3)
    want = reference(oracle, [stores], [0], [0], qv, np.zeros((2, 1), F32), np.ones((2, 1), F32), 5, 3)
    check(got, want, 3, "after errors")


def test_full_size_config5_store():
    """config 5's store (1M x 768, cosine), 1024 queries, cand_size 20, k_out 11: 16 sampled
    queries against numpy"""
    import searchlite_amd as sa
    from searchlite_amd import corpus
    n, dim, nq = 1_000_000, 768, 1024
    vals = corpus.unit_vectors(n, dim, seed=11)
    offs = np.arange(n, dtype=np.uint32)
    qv = corpus.unit_vectors(nq, dim, seed=12)
    with sa.GpuIndex([_seg(n, offs, vals)]) as ix:
        doc, seg, score, vec, count, total = _run(ix, [0], qv, 0.0, 20, 11)
    assert np.all(count == 11) and np.all(total == 20) and np.all(seg == 0)
    for q in np.random.default_rng(0).choice(nq, 16, replace=False):
        s = vals @ qv[q]
        order = np.lexsort((np.arange(n), -s))[:11]
        assert np.abs(score[q] - s[order]).max() <= TOL
        assert np.abs(vec[q] - s[order]).max() <= TOL
        for i in range(11):
            if doc[q, i] != order[i]:
                assert abs(s[doc[q, i]] - s[order[i]]) <= 2 * TOL
