"""Two-pass vector search on the device (slg_index_quantize_vector_field, slg_vector_search_batch_approx*): the
bf16 copy bit for bit against a numpy restatement of round-to-nearest-even, and the search against the exact call
(slg_vector_search_batch) on the same index.  Every returned score of the two-pass call is the exact call's, so
whenever the first pass must hand the second one the exact call's clause lists the whole output is byte-identical:
  - bf16-exact worlds (components k/16, |k| <= 8: every value is a bf16 value and every product and partial sum is
    exact in f32 in any order), where the first pass reproduces the exact ranking with all its ties;
  - refine >= the live docs with a vector, whatever the first pass computes;
  - planted score gaps wider than twice the first pass's error bound (cosine of unit vectors: both operands carry a
    relative rounding error <= 2^-9, Cauchy-Schwarz bounds the summed products by 1, the f32 accumulation over at most
    1024 dimensions adds < 2^-14: below 2^-7 * |boost|; the gaps asserted are 2^-6 * |boost|.  L2: the squared
    distance |x|^2 + |q|^2 - 2 x.q errs by twice the dot's bound, 2^-7 * |x| |q|; the gap asserted is 2^-5 * max|x| |q|).
On general data only the per-row facts hold: exact scores, the order, the counts.  No recall is asserted."""
import numpy as np
import pytest

from tests.test_gpu_vector_search import NOVEC, _seg, _store, _tkey, _unit, check, reference

pytestmark = pytest.mark.gpu
F32 = np.float32


def bf16_rne(x):
    """f32 array -> bf16 bit patterns, round to nearest even (NaN lanes: see is_nan16)"""
    b = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def is_nan16(h):
    return ((h & 0x7F80) == 0x7F80) & ((h & 0x007F) != 0)


def norms_l2r(vals):
    """left-to-right f32 sum of squares of each row"""
    out = np.zeros(len(vals), F32)
    with np.errstate(all="ignore"):
        for k in range(vals.shape[1]):
            out = (out + (vals[:, k] * vals[:, k]).astype(F32)).astype(F32)
    return out


def check_copy(got, vals, what):
    bits, norms = got
    assert bits.shape == vals.shape and norms.shape == (len(vals),), what
    want = bf16_rne(vals)
    nan = np.isnan(vals)
    assert np.array_equal(bits[~nan], want[~nan]), what
    assert is_nan16(bits[nan]).all(), f"{what}: a NaN did not stay a NaN"
    wn = norms_l2r(vals)
    assert np.array_equal(np.isnan(norms), np.isnan(wn)), what
    ok = ~np.isnan(wn)
    assert np.array_equal(norms[ok].view(np.uint32), wn[ok].view(np.uint32)), f"{what}: norms"


def same(got, want, what):
    for name, a, b in zip(("doc", "seg", "score", "vec", "count", "total"), got, want):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), \
            f"{what}: {name} differs from the exact call"


SPECIAL = np.array([0x00000000, 0x80000000,               # +-0
                    0x00000001, 0x80000001, 0x00012345, 0x007FFFFF, 0x00008000, 0x00018000,  # denormals (two halfway)
                    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # halfway: even / odd lower neighbour
                    0x3F808001, 0x3F807FFF, 0x3F817FFF,               # just above / below halfway
                    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000,  # largest finite -> inf; below; halfway -> inf
                    0x7F800000, 0xFF800000,                           # +-inf
                    0x7FC00000, 0x7F800001, 0xFFC12345, 0x7F80FFFF],  # NaNs (two with the payload in the low half)
                   np.uint32).view(F32)


@pytest.mark.parametrize("dim", [1, 7, 8, 9, 33])
def test_quantize_bit_for_bit(dim):
    import searchlite_amd as sa
    rng = np.random.default_rng(dim)

    def rows(n, d):
        v = rng.standard_normal((n, d)).astype(F32)
        flat = v.reshape(-1)
        pos = rng.choice(flat.size, size=min(flat.size, 3 * len(SPECIAL)), replace=flat.size < 3 * len(SPECIAL))
        flat[pos] = SPECIAL[np.arange(len(pos)) % len(SPECIAL)]
        return v
    n0 = 90
    have = rng.random(n0) < 0.6
    offs = np.full(n0, NOVEC, np.uint32)
    offs[have] = rng.permutation(int(have.sum()))
    v0 = rows(int(have.sum()), dim)
    v2 = rows(37, dim + 1)                       # a segment of another dimension
    v3 = rows(300, dim)                          # more rows than one workgroup takes
    segs = [_seg(n0, offs, v0), _seg(25), _seg(37, np.arange(37), v2), _seg(300, np.arange(300)[::-1].copy(), v3)]
    with sa.GpuIndex(segs) as ix:
        ix.quantize_vector_field(0)
        ix.quantize_vector_field(0)              # a no-op
        check_copy(ix.fetch_vector_copy(0, 0, dim), v0, f"dim {dim} seg 0")
        assert ix.fetch_vector_copy(0, 1, dim) is None      # the segment without the field
        check_copy(ix.fetch_vector_copy(0, 2, dim + 1), v2, f"dim {dim} seg 2")
        check_copy(ix.fetch_vector_copy(0, 3, dim), v3, f"dim {dim} seg 3")


def _grid(rng, shape):
    return (rng.integers(-8, 9, size=shape) / 16.0).astype(F32)


DIMS, DOCS, NQS, CANDS = [1, 3, 31, 32, 33, 64, 100], [127, 128, 129, 300], [1, 63, 64, 65], [1, 32, 33, 64, 65, 200]
EXACT_CASES = [(m, DIMS[i % 7], DOCS[i % 4], NQS[(i + i // 4) % 4], CANDS[i % 6]) for m in (0, 1) for i in range(12)]


@pytest.mark.parametrize("metric,dim,docs,nq,cand", EXACT_CASES)
def test_bf16_exact_worlds_are_byte_identical_at_refine_equal_cand(metric, dim, docs, nq, cand):
    import searchlite_amd as sa
    rng = np.random.default_rng(1000 * metric + 7 * dim + docs + nq + cand)
    n_segs = 2 + (docs + dim) % 2
    sizes = [docs // n_segs] * (n_segs - 1)
    sizes.append(docs - sum(sizes))
    stores = [_store(rng, n, dim, metric, p_missing=0.15, values=_grid(rng, (n, dim))) for n in sizes]
    qv = _grid(rng, (nq, dim))
    for variant in (0, 1):
        segs = [_seg(n, st[1], st[2], metric=metric) for n, st in zip(sizes, stores)]
        boost, q_filter, masks = None, None, None
        if variant:
            for s, n in enumerate(sizes):
                segs[s].set_deleted(rng.choice(n, size=n // 7, replace=False).tolist())
            boost = rng.choice(np.array([1.0, -1.0, 0.5], F32), size=(nq, 1))
            masks = [rng.random(n) < 0.6 for n in sizes]
            q_filter = np.where(rng.random(nq) < 0.5, 0, -1).astype(np.int32)
        with sa.GpuIndex(segs) as ix:
            if masks is not None:
                assert ix.add_filter(masks) == 0
            ix.quantize_vector_field(0)
            k_out = min(cand + 1, docs)
            want = ix.vector_search([0], qv, 0.0, cand, k_out, boost=boost, q_filter=q_filter)
            got = ix.vector_search_approx([0], qv, 0.0, cand, cand, k_out, boost=boost, q_filter=q_filter)
        same(got, want, f"metric {metric} dim {dim} docs {docs} nq {nq} cand {cand} variant {variant}")
        assert int(want[4].max()) > 0


def _fields_world(rng, n_docs, fdims, fmetrics):
    fields = [[_store(rng, n, d, m, p_missing=0.25) for n in n_docs] for d, m in zip(fdims, fmetrics)]
    fields[2][1] = None  # a segment without field 2
    return fields


@pytest.mark.parametrize("n_docs,refine", [((260, 180), 440), ((260, 180), 10000), ((30, 25), 64), ((30, 25), 56)])
@pytest.mark.parametrize("clause_field", [[0], [3], [1, 2], [0, 3, 2]])
def test_refine_of_all_docs_is_byte_identical_on_random_data(n_docs, refine, clause_field):
    """pins vs_refine_kernel's arithmetic to the scan's, whatever the first pass does: dims 5, 36, 100, 257 put the
    fmaf chain past one 32-step and past a padded tail"""
    import searchlite_amd as sa
    rng = np.random.default_rng(sum(n_docs) + refine + 31 * len(clause_field) + clause_field[0])
    fdims, fmetrics = [36, 100, 257, 5], [0, 1, 0, 1]
    fields = _fields_world(rng, n_docs, fdims, fmetrics)
    nq, nc = 9, len(clause_field)
    qv = np.concatenate([_unit(rng, nq, fdims[f]) if fmetrics[f] == 0 else
                         rng.standard_normal((nq, fdims[f])).astype(F32) for f in clause_field], axis=1)
    alpha = np.zeros((nq, nc), F32)
    alpha[1], alpha[2], alpha[3, 0] = 1.0, 0.3, 0.75
    alpha[4] = np.linspace(0.0, 1.0, nc, dtype=F32)
    boost = np.ones((nq, nc), F32)
    boost[5], boost[6, 0] = 1.5, -2.0
    segs = [_seg(n, *fields[0][s][1:]) for s, n in enumerate(n_docs)]
    segs[0].set_deleted([1, 5, 17])
    with sa.GpuIndex(segs) as ix:
        for f in (1, 2, 3):
            assert ix.add_vector_field(fields[f]) == f
        for f in set(clause_field):
            ix.quantize_vector_field(f)
        for cand in (10, min(70, refine)):
            k_out = cand + 3
            want = ix.vector_search(clause_field, qv, alpha, cand, k_out, boost=boost)
            got = ix.vector_search_approx(clause_field, qv, alpha, cand, refine, k_out, boost=boost)
            same(got, want, f"fields {clause_field} docs {n_docs} refine {refine} cand {cand}")


def _exact_sorted(oracle, stores, metric, qv, boost):
    """per query the oracle's boosted scores of every doc with a vector, best first"""
    nq = len(qv)
    n_all = sum(len(st[1]) for st in stores)
    ref = reference(oracle, [stores], [metric], [0], qv, np.zeros((nq, 1), F32), boost, n_all, 1)
    return [sorted((float(v) for v in maps[0].values()), reverse=True) for _, _, maps in ref]


@pytest.mark.parametrize("dim", [33, 100])
@pytest.mark.parametrize("refine", [20, 40, 64, 65])
def test_planted_cosine_gaps_are_byte_identical(oracle, dim, refine):
    import searchlite_amd as sa
    rng = np.random.default_rng(dim)
    cand, nq, sizes = 20, 5, (280, 220)
    qv = _unit(rng, nq, dim)
    boost = np.array([[1.0], [0.5], [2.0], [1.0], [0.5]], F32)
    stores = [_store(rng, n, dim, 0, p_missing=0.1) for n in sizes]
    vals = [st[2].copy() for st in stores]
    free = [list(rng.permutation(len(v))) for v in vals]  # rows not planted yet
    for q in range(nq):  # cand docs near the query, spread over both segments
        for j in range(cand):
            s = (q + j) % 2
            v = qv[q] + F32(0.3) * _unit(rng, 1, dim)[0]
            vals[s][free[s].pop()] = (v / np.linalg.norm(v)).astype(F32)
    stores = [(0, st[1], v) for st, v in zip(stores, vals)]
    # the gaps, from the oracle's scores, before anything touches the device
    for q, sc in enumerate(_exact_sorted(oracle, stores, 0, qv, boost)):
        bound = 2.0 ** -6 * abs(float(boost[q, 0]))
        assert sc[cand - 1] - sc[cand] > bound, f"q{q}: no gap at the cand_size boundary"
        assert sc[cand - 1] - sc[refine] > bound, f"q{q}: no gap at the refine boundary"
    segs = [_seg(n, st[1], st[2]) for n, st in zip(sizes, stores)]
    with sa.GpuIndex(segs) as ix:
        ix.quantize_vector_field(0)
        want = ix.vector_search([0], qv, 0.0, cand, cand + 1, boost=boost)
        got = ix.vector_search_approx([0], qv, 0.0, cand, refine, cand + 1, boost=boost)
    same(got, want, f"planted cosine dim {dim} refine {refine}")


@pytest.mark.parametrize("dim", [33, 100])
@pytest.mark.parametrize("refine", [20, 40, 64, 65])
def test_planted_l2_near_duplicates_are_byte_identical(oracle, dim, refine):
    import searchlite_amd as sa
    rng = np.random.default_rng(100 + dim)
    cand, nq, sizes = 20, 4, (280, 220)
    qv = rng.standard_normal((nq, dim)).astype(F32)
    boost = np.ones((nq, 1), F32)
    stores = [_store(rng, n, dim, 1, p_missing=0.1) for n in sizes]
    vals = [st[2].copy() for st in stores]
    free = [list(rng.permutation(len(v))) for v in vals]  # rows not planted yet
    for q in range(nq):
        for j in range(cand):
            s = (q + j) % 2
            eps = F32(10.0 ** -rng.uniform(1, 4))
            vals[s][free[s].pop()] = (qv[q] + eps * _unit(rng, 1, dim)[0]).astype(F32)
    stores = [(1, st[1], v) for st, v in zip(stores, vals)]
    xmax = max(float(np.linalg.norm(v.astype(np.float64), axis=1).max()) for v in vals)
    for q, sc in enumerate(_exact_sorted(oracle, stores, 1, qv, boost)):
        bound = 2.0 ** -5 * xmax * float(np.linalg.norm(qv[q].astype(np.float64)))
        d2 = [s * s for s in sc]  # squared distances, ascending
        assert d2[cand] - d2[cand - 1] > bound, f"q{q}: no gap at the cand_size boundary"
        assert d2[refine] - d2[cand - 1] > bound, f"q{q}: no gap at the refine boundary"
    segs = [_seg(n, st[1], st[2], metric=1) for n, st in zip(sizes, stores)]
    with sa.GpuIndex(segs) as ix:
        ix.quantize_vector_field(0)
        want = ix.vector_search([0], qv, 0.0, cand, cand + 1, boost=boost)
        got = ix.vector_search_approx([0], qv, 0.0, cand, refine, cand + 1, boost=boost)
    same(got, want, f"planted l2 dim {dim} refine {refine}")


@pytest.mark.parametrize("metric,dim,cand,refine", [(0, 48, 10, 16), (0, 200, 33, 64), (0, 48, 10, 100),
                                                    (1, 48, 10, 16), (1, 200, 64, 65), (1, 48, 70, 150)])
def test_general_data_rows_carry_exact_scores_in_order(metric, dim, cand, refine):
    import searchlite_amd as sa
    rng = np.random.default_rng(dim + cand + refine + metric)
    sizes = (300, 260)
    n_all = sum(sizes)
    stores = [_store(rng, n, dim, metric, p_missing=0.1) for n in sizes]
    segs = [_seg(n, st[1], st[2], metric=metric) for n, st in zip(sizes, stores)]
    nq, k_out = 7, cand
    qv = _unit(rng, nq, dim) if metric == 0 else rng.standard_normal((nq, dim)).astype(F32)
    alpha = np.zeros((nq, 1), F32)
    alpha[3:] = 0.3
    with sa.GpuIndex(segs) as ix:
        ix.quantize_vector_field(0)
        edoc, eseg, esc, evec, ecnt, _ = ix.vector_search([0], qv, alpha, n_all, n_all)
        doc, seg, sc, vec, cnt, tot = ix.vector_search_approx([0], qv, alpha, cand, refine, k_out)
    for q in range(nq):
        exact = {(int(eseg[q, i]), int(edoc[q, i])): (esc[q, i].tobytes(), evec[q, i].tobytes())
                 for i in range(int(ecnt[q]))}
        assert int(tot[q]) == cand and int(cnt[q]) == min(k_out, cand)
        rows = [(int(seg[q, i]), int(doc[q, i])) for i in range(int(cnt[q]))]
        assert len(set(rows)) == len(rows)
        for i, key in enumerate(rows):
            assert exact[key] == (sc[q, i].tobytes(), vec[q, i].tobytes()), f"q{q} row {i}: not the exact score"
        order = [(-_tkey(sc[q, i]), rows[i][0], rows[i][1]) for i in range(len(rows))]
        assert order == sorted(order), f"q{q}: rows out of order"
        assert np.all(doc[q, len(rows):] == 0) and np.all(sc[q, len(rows):] == 0)


def test_lifecycle_and_device_form():
    import torch
    import searchlite_amd as sa
    rng = np.random.default_rng(77)
    dim, d1 = 40, 12
    stores = [_store(rng, 300, dim, 0), _store(rng, 200, dim, 0)]
    segs = [_seg(300, *stores[0][1:]), _seg(200, *stores[1][1:])]
    nq, cand, k_out, R = 6, 15, 16, 1000
    qv = _unit(rng, nq, dim)

    def both(ix, what, cf=(0,), q=qv, **kw):
        want = ix.vector_search(list(cf), q, 0.2, cand, k_out, **kw)
        got = ix.vector_search_approx(list(cf), q, 0.2, cand, R, k_out, **kw)
        same(got, want, what)
        return got
    with sa.GpuIndex(segs) as ix:
        fid = ix.add_filter([rng.random(300) < 0.5, rng.random(200) < 0.5])
        ix.quantize_vector_field(0)
        flt = np.array([fid, -1] * 3, np.int32)
        got = both(ix, "quantised", q_filter=flt)
        # tombstones: nothing to redo, the next call follows the new state
        bits = np.zeros(300, bool)
        bits[[int(d) for q in range(nq) for d, s in zip(got[0][q, :3], got[1][q, :3]) if s == 0] + [1, 2]] = True
        ix.update_deleted(0, np.packbits(bits, bitorder="little"), float(300 - bits.sum()))
        both(ix, "update_deleted", q_filter=flt)
        # a new segment: its field-0 store is quantised by the update
        st2 = _store(rng, 150, dim, 0)
        assert ix.add_segment(_seg(150, *st2[1:])) == 2
        check_copy(ix.fetch_vector_copy(0, 2, dim), st2[2], "added segment")
        both(ix, "add_segment")
        ix.remove_segment(0)
        check_copy(ix.fetch_vector_copy(0, 0, dim), stores[1][2], "after remove_segment: old segment 1")
        check_copy(ix.fetch_vector_copy(0, 1, dim), st2[2], "after remove_segment: the added segment")
        both(ix, "remove_segment")
        # a field added after the first quantise
        f1 = [_store(rng, 200, d1, 1), None]
        assert ix.add_vector_field(f1) == 1
        with pytest.raises(sa._native.SlgError):
            ix.vector_search_approx([0, 1], np.zeros((1, dim + d1), F32), 0.0, 1, 1, 1)
        ix.quantize_vector_field(1)
        check_copy(ix.fetch_vector_copy(1, 0, d1), f1[0][2], "field 1")
        assert ix.fetch_vector_copy(1, 1, d1) is None
        q2 = np.concatenate([qv, rng.standard_normal((nq, d1)).astype(F32)], axis=1)
        boost = np.full((nq, 2), 1.5, F32)
        want = both(ix, "two fields", cf=(0, 1), q=q2, boost=boost)
        # the _device form
        dev = torch.device("cuda", 0)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        dq, da, db = t(q2), t(np.full((nq, 2), 0.2, F32)), t(boost)
        od = torch.zeros((nq, k_out), dtype=torch.int32, device=dev)
        os_, osc, ov = torch.zeros_like(od), torch.zeros((nq, k_out), device=dev), torch.zeros((nq, k_out), device=dev)
        oc = torch.zeros(nq, dtype=torch.int32, device=dev)
        ot = torch.zeros(nq, dtype=torch.int64, device=dev)
        for refine in (cand, 64, R):
            host = ix.vector_search_approx([0, 1], q2, 0.2, cand, refine, k_out, boost=boost)
            ix.vector_search_approx_device(nq, [0, 1], dq.data_ptr(), da.data_ptr(), db.data_ptr(), None, cand, refine,
                                           k_out, od.data_ptr(), os_.data_ptr(), osc.data_ptr(), ov.data_ptr(),
                                           oc.data_ptr(), ot.data_ptr())
            torch.cuda.synchronize()
            same([x.cpu().numpy() for x in (od, os_, osc, ov, oc, ot)], host, f"device form, refine {refine}")
        same(host, want, "device form's host twin")


def test_error_codes_then_a_valid_call(oracle):
    import searchlite_amd as sa
    from searchlite_amd import _native as N
    rng = np.random.default_rng(3)
    dim = 8
    stores = [_store(rng, 100, dim, 0)]
    qv = _unit(rng, 2, dim)
    lib = N.load()
    with sa.GpuIndex([_seg(100, *stores[0][1:])]) as ix:
        def rc(fn, *a, **kw):
            try:
                fn(*a, **kw)
            except N.SlgError as e:
                return e.code, str(e)
            return 0, ""
        code, msg = rc(ix.vector_search_approx, [0], qv, 0.0, 5, 8, 3)
        assert code == N.ERR_INVALID and "field 0" in msg          # no copy yet
        assert rc(ix.quantize_vector_field, 1)[0] == N.ERR_INVALID  # no such field
        assert rc(ix.fetch_vector_copy, 0, 0, dim)[0] == N.ERR_INVALID  # no copy to fetch
        ix.quantize_vector_field(0)
        assert rc(ix.fetch_vector_copy, 0, 1, dim)[0] == N.ERR_INVALID  # no such segment
        assert rc(ix.vector_search_approx, [0], qv, 0.0, 5, 4, 3)[0] == N.ERR_UNSUPPORTED
        assert rc(ix.vector_search_approx, [0], qv, 0.0, 5, 10001, 3)[0] == N.ERR_UNSUPPORTED
        assert rc(ix.vector_search_approx, [0], qv, 0.0, 0, 0, 3)[0] == N.ERR_UNSUPPORTED
        assert rc(ix.vector_search_approx, [0], qv, 0.0, 5, 8, 20002)[0] == N.ERR_UNSUPPORTED
        assert rc(ix.vector_search_approx, [3], qv, 0.0, 5, 8, 3)[0] == N.ERR_INVALID
        assert rc(ix.vector_search_approx, [0], qv, 0.0, 5, 8, 3,
                  q_filter=np.array([0, -1], np.int32))[0] == N.ERR_INVALID  # no such filter (host form)
        cf = np.zeros(1, np.uint32)
        assert lib.slg_vector_search_batch_approx(ix._h, 2, 1, cf.ctypes.data, None, None, None, None, 5, 8, 3,
                                                  None, None, None, None, None, None) == N.ERR_INVALID
        # nq = 0 returns 0 and writes nothing
        cnt = np.full(2, 7, np.uint32)
        assert lib.slg_vector_search_batch_approx(ix._h, 0, 1, cf.ctypes.data, None, None, None, None, 5, 8, 3,
                                                  None, None, None, None, cnt.ctypes.data, None) == 0
        assert (cnt == 7).all()
        got = ix.vector_search_approx([0], qv, 0.0, 5, 100, 3)  # (refine = every doc)
        same(got, ix.vector_search([0], qv, 0.0, 5, 3), "after errors")
    want = reference(oracle, [stores], [0], [0], qv, np.zeros((2, 1), F32), np.ones((2, 1), F32), 5, 3)
    check(got, want, 3, "after errors")
