"""The three rerank kernels (rerank_kernel, rerank_multi_kernel, rerank_fields_kernel) at every top-k
register width, at their candidate limits, over candidates from several segments, and at value edges.

Two kinds of data:
  - "int": vectors of small integers.  Every product and sum of a similarity is exact in f32 whatever
    the order (lane-parallel sums, matrix cores, the L2 identity), so with alpha = 1 (the blend is the
    bm25 bits), alpha = 0 (the similarity, or runs of -1.0 / f32::MIN for missing vectors) and the
    mixed alphas of the f32 blend, the kernels must match the oracle bit for bit (assert_same_hits).
    bm25 values are quarters, so exact ties fall across the k cut, inside one segment and across them.
  - "real": unit cosine vectors and L2 vectors whose norms run from 1e-3 to 1e3, mixed alphas (0, 1,
    just inside both, outside [0, 1]); checked against the float64 intervals of tests.util.rerank_exact
    by check_rerank_result (order, membership, scores in bound, nothing better left out).

Candidates come from three segments, include docs past their segment's n_docs and segments >= n_segs
(candidates without a vector), and the oracle runs on combined ids (tests.util.oracle_rerank_segments).

Failures these tests found, fixed with them:
  - A segment without vectors was staged with its descriptor's unchecked vec_metric (0, cosine, by
    default), and a candidate whose segment is >= n_segs took metric 0 in rerank_kernel: on an L2 field
    such candidates scored -1.0 instead of f32::MIN and ranked above every L2 hit farther than 1
    (test_rerank_vectorless_segment[...l2], test_rerank_segment_out_of_range).
  - rerank_kernel stored a blend of -0.0 as the score; the reference adds it to 0.0 (api/reader.rs:232,
    249), so it scores +0.0 and ties with +0.0 by (seg, doc) (test_rerank_bm25_specials[one]).

Out of scope: L2 rows, queries or alphas whose blend is NaN (the sign of an arithmetic NaN differs
between x86 and gfx950, so the reference itself is platform-defined there); sums that overflow in one
order and not in another; sorted batches passed to slg_batch_rerank_device."""
import functools
import zlib

import numpy as np
import pytest

from tests.util import (F32_MAX, NO_VECTOR, TOPK_WIDTH_KS, assert_same_hits, check_rerank_result,
                        oracle_rerank_segments, random_segment)

pytestmark = pytest.mark.gpu

MAX_RERANK_K = 1024
RERANK_KS = tuple(k for k in TOPK_WIDTH_KS if k <= MAX_RERANK_K)
SEG_DOCS = (700, 900, 500)
K_MULTI_LDS_FLOATS = 36 * 1024

# path -> (kind, [(field, dim, metric) per clause]).  Field 0 is the segment descriptors' field; the
# fields kernel adds fields 1 and 2.  Per kernel the path the dims take (slg_rerank.hpp):
#   one:    whole rows of 1 / 2 / 3 chunks (dim % 4 == 0, <= 256 / 512 / 768), generic loop (dim % 4 != 0
#           or dim > 768)
#   multi:  matrix cores (cosine, dim % 16 == 0), VALU rows (dim % 4 == 0, <= 768), registers
#           (dim <= 1024), streaming (dim > 1024), L2 on the matrix-core identity (>= 3 clauses)
#   fields: fast clauses (96-d at offset 0, 40-d at 96) and slow ones (6-d: dim % 4; 96-d at offset 142)
PATHS = {
    "one-rows1-cos": ("one", [(0, 64, 0)]),
    "one-rows2-l2": ("one", [(0, 384, 1)]),
    "one-rows3-cos": ("one", [(0, 768, 0)]),
    "one-generic-dim102-l2": ("one", [(0, 102, 1)]),
    "one-generic-dim1030-cos": ("one", [(0, 1030, 0)]),
    "multi-mfma-cos": ("multi", [(0, 64, 0)] * 2),
    "multi-valu-rows-l2": ("multi", [(0, 100, 1)] * 2),
    "multi-registers-cos": ("multi", [(0, 102, 0)] * 2),
    "multi-streaming-cos": ("multi", [(0, 1100, 0)] * 2),
    "multi-l2-identity": ("multi", [(0, 64, 1)] * 3),
    "fields-fast-slow": ("fields", [(0, 96, 0), (1, 40, 1), (2, 6, 1), (0, 96, 0)]),
}


def _kind(path):
    return PATHS[path][0]


def _l2_identity(path):
    kind, cl = PATHS[path]
    return kind == "multi" and cl[0][2] == 1 and len(cl) >= 3 and cl[0][1] % 16 == 0


def _vectors(rng, n, dim, metric, data):
    if data == "int":
        return rng.integers(-2, 3, size=(n, dim)).astype(np.float32)
    v = rng.normal(size=(n, dim))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if metric == 1:
        v *= 10.0 ** rng.uniform(-3, 3, size=(n, 1))
    return v.astype(np.float32)


def _field(rng, dim, metric, data, seg_docs=SEG_DOCS, vectorless=()):
    segs = []
    for s, n in enumerate(seg_docs):
        if s in vectorless:
            segs.append(None)
            continue
        offs = rng.permutation(n).astype(np.uint32)
        offs[rng.random(n) < 0.3] = NO_VECTOR
        segs.append((offs, _vectors(rng, n, dim, metric, data)))
    return dict(metric=metric, dim=dim, segs=segs)


@functools.lru_cache(maxsize=None)
def _fields(path, data, seg_docs=SEG_DOCS, vectorless=()):
    """The fields of a path: field f has the dim and metric its clauses name."""
    rng = np.random.default_rng(zlib.crc32(repr((path, data, seg_docs, vectorless)).encode()))
    spec = {}
    for f, dim, metric in PATHS[path][1]:
        spec[f] = (dim, metric)
    return [_field(rng, *spec[f], data, seg_docs, vectorless) for f in sorted(spec)]


def _pool(seg_docs, n_segs_extra=True):
    """Every (seg, doc) a candidate may be: the segments' docs, 8 past each segment's n_docs, and 40 docs
    of segment n_segs (out of range)."""
    seg, doc = [], []
    for s, n in enumerate(seg_docs):
        seg += [s] * (n + 8)
        doc += list(range(n + 8))
    if n_segs_extra:
        seg += [len(seg_docs)] * 40
        doc += list(range(40))
    return np.array(seg, np.uint32), np.array(doc, np.uint32)


def _segments(fields, seg_docs):
    """Segments carrying field 0 (a segment without it: vec_dim 0 and the default vec_metric 0)."""
    from searchlite_amd.segment import Segment
    out = []
    for s, n in enumerate(seg_docs):
        sd = fields[0]["segs"][s]
        kw = {} if sd is None else dict(vec_dim=fields[0]["dim"], vec_metric=fields[0]["metric"],
                                        vec_offsets=sd[0], vec_values=sd[1])
        out.append(Segment(n_docs=n, term_offsets=[0, 1], doc_ids=[0], tfs=[1],
                           field_doc_len=[np.ones(n, np.float32)], field_avgdl=[1.0], docs=float(n), **kw))
    return out


def _queries(rng, path, fields, counts, max_cand, alpha_mode, data, seg_docs=SEG_DOCS, bm=None):
    kind, cl = PATHS[path]
    nc = len(cl)
    ps, pd = _pool(seg_docs)
    qs = []
    for cnt in counts:
        pick = rng.choice(len(ps), size=max_cand, replace=False)
        if alpha_mode == "one":
            alpha = np.ones(nc, np.float32)
        elif alpha_mode == "zero":
            alpha = np.zeros(nc, np.float32)
        else:
            alpha = rng.choice(np.array([0.0, 1.0, 2.0 ** -24,
                                         np.nextafter(np.float32(1), np.float32(0)), -0.5, 1.5, 0.3, 0.7],
                                        np.float32), size=nc)
        boost = None if kind == "one" else rng.choice(np.array([0.5, 1.5, 2.0], np.float32), size=nc)
        q = dict(cf=[f for f, _, _ in cl], alpha=alpha, boost=boost,
                 qv=[_vectors(rng, 1, dim, metric, data)[0] for _, dim, metric in cl],
                 seg=ps[pick], doc=pd[pick],
                 bm=(rng.integers(0, 24, size=max_cand) / 4).astype(np.float32) if bm is None else bm(max_cand),
                 count=cnt)
        qs.append(q)
    return qs


def _run(ix, path, qs, k_out, field_ids=None):
    """One host-entry call for the batch of queries qs -> (doc, seg, score, vec, count)."""
    kind, cl = PATHS[path]
    cd = np.stack([q["doc"] for q in qs])
    cs = np.stack([q["seg"] for q in qs])
    bm = np.stack([q["bm"] for q in qs])
    cnt = np.array([q["count"] for q in qs], np.uint32)
    alpha = np.stack([q["alpha"] for q in qs])
    if kind == "one":
        return ix.rerank_batch(np.stack([q["qv"][0] for q in qs]), alpha[:, 0], cd, cs, bm, cnt, k_out)
    boost = np.stack([q["boost"] for q in qs])
    if kind == "multi":
        return ix.rerank_multi_batch(np.stack([np.stack(q["qv"]) for q in qs]), alpha, cd, cs, bm, cnt, k_out,
                                     boost=boost)
    qcat = np.stack([np.concatenate(q["qv"]) for q in qs])
    return ix.rerank_fields_batch([field_ids[f] for f in qs[0]["cf"]], qcat, alpha, cd, cs, bm, cnt, k_out,
                                  boost=boost)


def _index(sa, fields, seg_docs=SEG_DOCS):
    """-> (GpuIndex, field ids): field 0 in the segment descriptors, the others added."""
    ix = sa.GpuIndex(_segments(fields, seg_docs))
    ids = [0]
    for f in fields[1:]:
        ids.append(ix.add_vector_field([None if sd is None else (f["metric"], sd[0], sd[1]) for sd in f["segs"]]))
    return ix, ids


def _truncated(q):
    n = q["count"]
    return dict(q, seg=q["seg"][:n], doc=q["doc"][:n], bm=q["bm"][:n])


def _assert_oracle_bits(oracle, path, fields, qs, k_out, got, what):
    """got against the oracle on every query: (seg, doc) sequence and score bits identical, vector scores
    equal."""
    kind = _kind(path)
    nq = len(qs)
    wd = np.zeros((nq, k_out), np.uint32)
    ws = np.zeros((nq, k_out), np.uint32)
    wsc = np.zeros((nq, k_out), np.float32)
    wc = np.zeros(nq, np.uint32)
    for i, q in enumerate(qs):
        d, s, sc, v = oracle_rerank_segments(oracle, fields, _truncated(q), kind, k_out)
        n = len(d)
        wd[i, :n], ws[i, :n], wsc[i, :n], wc[i] = d, s, sc, n
        gv = got[3][i, :n]
        assert np.array_equal(gv, v) or np.array_equal(gv.view(np.uint32), v.view(np.uint32)), \
            f"{what}: query {i} vector scores differ at {int(np.argmax(gv != v))}"
    assert_same_hits((got[0], got[1], got[2], got[4]), (wd, ws, wsc, wc), what=what)


def _counts(k_out, max_cand):
    return sorted({0, k_out - 1, k_out, k_out + 1, max_cand})


@pytest.mark.parametrize("k_out", RERANK_KS)
@pytest.mark.parametrize("path", list(PATHS))
def test_rerank_width_matrix(oracle, path, k_out):
    """Every kernel path x every top-k register width (KREGS 1 / 2 / 4 / 8 / 16 for k_out <= 64 / 128 /
    256 / 512 / 1024): candidate counts 0, k_out - 1, k_out, k_out + 1 and max_cand.  Integer data at
    alpha 1, 0 and mixed: bit for bit against the oracle; real data at mixed alphas: inside the float64
    bound."""
    import searchlite_amd as sa
    max_cand = k_out + 40
    rng = np.random.default_rng(1000 * k_out + len(path))
    for data, modes in (("int", ("one", "zero", "mixed")), ("real", ("mixed",))):
        fields = _fields(path, data)
        ix, ids = _index(sa, fields)
        with ix:
            for mode in modes:
                qs = _queries(rng, path, fields, _counts(k_out, max_cand), max_cand, mode, data)
                got = _run(ix, path, qs, k_out, ids)
                what = f"{path} k_out {k_out} {data} alpha {mode}"
                if data == "int":
                    _assert_oracle_bits(oracle, path, fields, qs, k_out, got, what)
                else:
                    for i, q in enumerate(qs):
                        check_rerank_result(fields, _truncated(q), _kind(path), k_out,
                                            tuple(a[i] for a in got), _l2_identity(path), f"{what} query {i}")


def _limit_max_cand(path):
    kind, cl = PATHS[path]
    nc = len(cl)
    if kind == "one":
        return 8192
    if kind == "multi":  # rerank_multi_lds_floats: nc (dim + 4) + nc max_cand + 2 max_cand + 8
        return (K_MULTI_LDS_FLOATS - nc * (cl[0][1] + 4) - 8) // (nc + 2)
    qf = sum(d for _, d, _ in cl)  # rerank_fields_lds_floats: round4(q_floats) + nc max_cand + 3 max_cand
    return (K_MULTI_LDS_FLOATS - ((qf + 3) & ~3)) // (nc + 3)


@pytest.mark.parametrize("path", ["one-rows1-cos", "multi-mfma-cos", "multi-l2-identity", "fields-fast-slow"])
def test_rerank_candidate_limit(oracle, path):
    """The largest max_cand a kernel's LDS takes (8192 for rerank_kernel, the exact fill of the 36 Ki-float
    budget for the others) is accepted and correct, at k_out 1024; one more is SLG_ERR_UNSUPPORTED."""
    import searchlite_amd as sa
    from searchlite_amd import _native as N
    mc = _limit_max_cand(path)
    seg_docs = (4200, 4200, 4200)
    assert sum(seg_docs) > mc + 1
    fields = _fields(path, "int", seg_docs)
    rng = np.random.default_rng(mc)
    ix, ids = _index(sa, fields, seg_docs)
    with ix:
        qs = _queries(rng, path, fields, [mc, 1000], mc, "mixed", "int", seg_docs)
        got = _run(ix, path, qs, 1024, ids)
        _assert_oracle_bits(oracle, path, fields, qs, 1024, got, f"{path} max_cand {mc}")
        qs = _queries(rng, path, fields, [mc + 1], mc + 1, "mixed", "int", seg_docs)
        with pytest.raises(N.SlgError) as e:
            _run(ix, path, qs, 1024, ids)
        assert e.value.code == N.ERR_UNSUPPORTED


@pytest.mark.parametrize("metric", [0, 1], ids=["cos", "l2"])
@pytest.mark.parametrize("path", ["one-rows1-cos", "one-generic-dim102-l2", "fields-fast-slow"])
def test_rerank_vectorless_segment(oracle, path, metric):
    """Segment 1 has no vectors in field 0 (its descriptor keeps vec_dim 0 and the default vec_metric 0):
    its candidates score missing_vector_score of the FIELD's metric, f32::MIN on an L2 field
    (api/reader.rs:217-223).  Before the fix they scored -1.0 there.  Fields kernel: field 0 takes the
    metric under test, segment 2 has no vectors in field 2."""
    import searchlite_amd as sa
    kind, cl = PATHS[path]
    rng = np.random.default_rng(77 + metric)
    fields = []
    dims = {}
    for f, dim, m in cl:
        dims[f] = (dim, metric if f == 0 else m)
    for f in sorted(dims):
        fields.append(_field(rng, *dims[f], "int", vectorless=(1,) if f == 0 else (2,) if f == 2 else ()))
    ix, ids = _index(sa, fields)
    with ix:
        for mode in ("zero", "mixed", "one"):
            for k_out in (10, 300):
                qs = _queries(rng, path, fields, [500, 1200, 37], 1200, mode, "int")
                got = _run(ix, path, qs, k_out, ids)
                _assert_oracle_bits(oracle, path, fields, qs, k_out, got,
                                    f"{path} vectorless segment metric {metric} alpha {mode} k_out {k_out}")


@pytest.mark.parametrize("path", ["one-rows1-cos", "one-generic-dim102-l2", "multi-mfma-cos",
                                  "multi-l2-identity", "fields-fast-slow"])
def test_rerank_segment_out_of_range(oracle, path):
    """Candidates whose segment is >= n_segs, or whose doc is >= its segment's n_docs, have no vector: at
    alpha 0 they form runs of the field's missing score, ordered by (seg, doc) — on L2 paths below every
    real hit, and only f32::MIN."""
    import searchlite_amd as sa
    fields = _fields(path, "int")
    rng = np.random.default_rng(5)
    ix, ids = _index(sa, fields)
    ps, pd = _pool(SEG_DOCS)
    off = np.array([s >= len(SEG_DOCS) or d >= SEG_DOCS[s] for s, d in zip(ps, pd)])
    with ix:
        qs = _queries(rng, path, fields, [150, 150], 150, "zero", "int")
        for q in qs:  # 110 candidates in range, 40 out of it
            pick = np.concatenate([rng.choice(np.flatnonzero(~off), size=110, replace=False),
                                   rng.choice(np.flatnonzero(off), size=40, replace=False)])
            rng.shuffle(pick)
            q["seg"], q["doc"] = ps[pick], pd[pick]
        got = _run(ix, path, qs, 140, ids)
        _assert_oracle_bits(oracle, path, fields, qs, 140, got, f"{path} out-of-range candidates")


BM_SPECIALS = [0.0, -0.0, np.inf, -np.inf, 3.0, -2.5]
NAN_BITS = [0x7FC00000, 0xFFC00000, 0xFFFFFFFF]


@pytest.mark.parametrize("path", ["one-rows1-cos", "one-generic-dim102-l2", "multi-mfma-cos",
                                  "multi-l2-identity", "fields-fast-slow"])
def test_rerank_bm25_specials(oracle, path):
    """bm25 of +-0 and +-inf under alpha >= 1 in all three kernels, and (rerank_kernel only, where the
    blended score is a plain copy) NaNs of either sign and the bits 0xFFFFFFFF — the smallest key of the
    total order, the same key as WaveTopK's sentinel — bit for bit against the oracle.  Before the fix
    rerank_kernel scored a bm25 of -0.0 as -0.0 (the reference: 0.0 + -0.0 = +0.0)."""
    import searchlite_amd as sa
    kind = _kind(path)
    specials = np.array(BM_SPECIALS, np.float32)
    if kind == "one":
        specials = np.concatenate([specials, np.array(NAN_BITS, np.uint32).view(np.float32)])

    def bm(n):
        return specials[np.arange(n) % len(specials)].copy()

    fields = _fields(path, "int")
    rng = np.random.default_rng(11)
    ix, ids = _index(sa, fields)
    with ix:
        for k_out in (5, 64, 200):
            qs = _queries(rng, path, fields, [300, 45], 300, "one", "int", bm=bm)
            if kind == "one":
                qs[1]["alpha"][:] = 1.5
            got = _run(ix, path, qs, k_out, ids)
            _assert_oracle_bits(oracle, path, fields, qs, k_out, got, f"{path} bm25 specials k_out {k_out}")


def _poison(fields, rng, what):
    """Copies of int fields where some rows hold NaN / +-inf / zeros (field 0 and, for the fields
    kernel, field 1)."""
    out = []
    for fi, f in enumerate(fields):
        segs = []
        for sd in f["segs"]:
            if sd is None:
                segs.append(None)
                continue
            o, v = sd[0], sd[1].copy()
            rows = rng.choice(len(v), size=len(v) // 10, replace=False)
            if fi == 0 and what == "nan":
                v[rows, rng.integers(0, v.shape[1], size=len(rows))] = np.nan
            elif fi == 0 and what == "inf":
                v[rows, rng.integers(0, v.shape[1], size=len(rows))] = np.where(rng.random(len(rows)) < 0.5,
                                                                              np.inf, -np.inf)
            elif fi == 0 and what == "zero":
                v[rows] = 0.0
            segs.append((o, v))
        out.append(dict(f, segs=segs))
    return out


@pytest.mark.parametrize("path,what", [(p, w) for p in ("one-rows1-cos", "one-generic-dim1030-cos", "one-rows2-l2",
                                                          "multi-mfma-cos", "multi-registers-cos", "multi-l2-identity",
                                                          "fields-fast-slow")
                                        for w in ("nan", "inf", "zero")
                                        if not (w == "nan" and PATHS[p][1][0][2] == 1)])  # (L2 NaN: out of scope)
def test_rerank_row_edges(oracle, path, what):
    """Rows holding a NaN, a +-inf, or all zeros (normalize_in_place leaves a zero row at zero), one row
    in ten — so an MFMA tile of 16 usually has 1 or 2 of them.  Cosine: NaN -> 0 (vectors/mod.rs:112-116)
    in the row scan, the generic loop and the matrix cores; +-inf rows give +-inf, or NaN -> 0 where the
    query element is 0 (single clause; with several clauses the query vectors are positive, so no clause
    sum adds +inf and -inf).  L2: NaN is out of scope (the NaN rows are skipped there); an inf row is -inf,
    below the f32::MIN of missing vectors.  Bit for bit against the oracle at alpha 0 and 1; a NaN in
    a query's clause vector scores every row 0."""
    import searchlite_amd as sa
    kind, cl = PATHS[path]
    rng = np.random.default_rng(zlib.crc32(what.encode()))
    fields = _poison(_fields(path, "int"), rng, what)
    ix, ids = _index(sa, fields)
    with ix:
        for mode in ("zero", "one"):
            qs = _queries(rng, path, fields, [400, 400, 129], 400, mode, "int")
            if what == "inf" and kind != "one":  # every clause over an inf row gets its sign: no inf - inf
                for q in qs:
                    q["qv"] = [np.abs(v) + 1 for v in q["qv"]]
            if what == "nan" and mode == "zero":
                qs[2]["qv"][0] = qs[2]["qv"][0].copy()
                qs[2]["qv"][0][3] = np.nan
            for k_out in (16, 129):
                got = _run(ix, path, qs, k_out, ids)
                _assert_oracle_bits(oracle, path, fields, qs, k_out, got, f"{path} {what} rows alpha {mode}")


def test_rerank_l2_near_overflow(oracle):
    """L2 on the matrix-core identity with values near f32 overflow: |q|^2 + |x|^2 overflows, so far rows
    score -inf (as the plain sum does) and an exact copy of the clause vectors takes the exact recompute
    (distance 0, the best score); checked against the float64 bound."""
    import searchlite_amd as sa
    path = "multi-l2-identity"
    rng = np.random.default_rng(3)
    scale = np.float32(3e18)
    f0 = _fields(path, "int")[0]
    fields = [dict(f0, segs=[(o, v * scale) for o, v in f0["segs"]])]
    qs = _queries(rng, path, fields, [300, 300], 300, "zero", "int")
    for q in qs:  # one vector for all three clauses, and an exact copy of it among the candidates
        v = q["qv"][0] * scale
        q["qv"] = [v, v, v]
        for s, d in zip(q["seg"], q["doc"]):
            if s < len(SEG_DOCS) and d < SEG_DOCS[s] and fields[0]["segs"][s][0][d] != NO_VECTOR:
                fields[0]["segs"][s][1][fields[0]["segs"][s][0][d]] = v
                break
    ix, ids = _index(sa, fields)
    with ix:
        got = _run(ix, path, qs, 50, ids)
    for i, q in enumerate(qs):
        check_rerank_result(fields, _truncated(q), "multi", 50, tuple(a[i] for a in got), True, f"query {i}")
        assert got[2][i, 0] == 0.0 and np.isneginf(got[2][i, 1]), f"query {i}"


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("path", ["one-rows3-cos", "multi-l2-identity", "fields-fast-slow"])
def test_rerank_device_entries_match_host(path):
    """slg_rerank_batch_device, slg_rerank_multi_batch_device and slg_rerank_fields_batch_device give the
    bits of their host entries (real data, mixed alphas, k_out 257)."""
    import torch
    import searchlite_amd as sa
    from searchlite_amd import _native as N
    kind, cl = PATHS[path]
    fields = _fields(path, "real")
    rng = np.random.default_rng(9)
    k_out, mc = 257, 600
    ix, ids = _index(sa, fields)
    with ix:
        qs = _queries(rng, path, fields, [600, 300, 256, 0], mc, "mixed", "real")
        want = _run(ix, path, qs, k_out, ids)
        nq = len(qs)
        cd = _dev(torch, np.stack([q["doc"] for q in qs]))
        cs = _dev(torch, np.stack([q["seg"] for q in qs]))
        bm = _dev(torch, np.stack([q["bm"] for q in qs]))
        cnt = _dev(torch, np.array([q["count"] for q in qs], np.uint32).view(np.int32))
        alpha = np.stack([q["alpha"] for q in qs])
        outs = [torch.zeros((nq, k_out), dtype=torch.int32, device="cuda"),
                torch.zeros((nq, k_out), dtype=torch.int32, device="cuda"),
                torch.zeros((nq, k_out), dtype=torch.float32, device="cuda"),
                torch.zeros((nq, k_out), dtype=torch.float32, device="cuda"),
                torch.zeros((nq,), dtype=torch.int32, device="cuda")]
        op = [t.data_ptr() for t in outs]
        cand = (cd.data_ptr(), cs.data_ptr(), bm.data_ptr(), cnt.data_ptr(), mc, k_out)
        keep = []
        if kind == "one":
            qv, a = _dev(torch, np.stack([q["qv"][0] for q in qs])), _dev(torch, alpha[:, 0].copy())
            keep += [qv, a]
            ix.rerank_batch_device(nq, qv.data_ptr(), a.data_ptr(), *cand, *op)
        elif kind == "multi":
            qv = _dev(torch, np.stack([np.stack(q["qv"]) for q in qs]))
            a, b = _dev(torch, alpha), _dev(torch, np.stack([q["boost"] for q in qs]))
            keep += [qv, a, b]
            ix.rerank_multi_batch_device(nq, len(cl), qv.data_ptr(), a.data_ptr(), b.data_ptr(), *cand, *op)
        else:
            cf = np.array([ids[f] for f in qs[0]["cf"]], np.uint32)
            qv = _dev(torch, np.stack([np.concatenate(q["qv"]) for q in qs]))
            a, b = _dev(torch, alpha), _dev(torch, np.stack([q["boost"] for q in qs]))
            keep += [qv, a, b]
            N.check(ix._lib.slg_rerank_fields_batch_device(
                ix._h, nq, len(cl), cf.ctypes.data, qv.data_ptr(), a.data_ptr(), b.data_ptr(), *cand, *op))
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in outs]
    for g, w, name in zip(got, want, ("doc", "seg", "score", "vec", "count")):
        if name == "count":
            assert np.array_equal(g.view(np.uint32), w), name
            continue
        for i in range(nq):
            n = int(want[4][i])
            assert np.array_equal(g[i, :n].view(np.uint32), np.asarray(w[i, :n]).view(np.uint32)), f"{name} query {i}"


@pytest.mark.parametrize("k_out", [10, 64, 65, 128, 129, 256, 257, 512, 513, 1024])
def test_batch_rerank_device_chain(oracle, k_out):
    """slg_batch_rerank_device on a two-segment BM25 batch (k = 1001, unsorted results) against the oracle
    chain search_batch -> rerank: integer vectors, alpha 0.5 / 0 / 1, so bit for bit."""
    import torch
    import searchlite_amd as sa
    from tests.util import random_queries
    rng = np.random.default_rng(42)
    segs = [random_segment(rng, n, 60, 8) for n in (2500, 1800)]
    dim = 64
    field = dict(metric=0, dim=dim, segs=[])
    for sg in segs:
        offs = rng.permutation(sg.n_docs).astype(np.uint32)
        offs[rng.random(sg.n_docs) < 0.2] = NO_VECTOR
        vals = rng.integers(-2, 3, size=(sg.n_docs, dim)).astype(np.float32)
        sg.vec_dim, sg.vec_metric, sg.vec_offsets, sg.vec_values = dim, 0, offs, vals
        field["segs"].append((offs, vals))
    nq, k = 6, 1001
    offs_q, terms, w = random_queries(rng, nq, 3, 60, n_segs=2)
    want = oracle.search_batch(segs, offs_q, terms, w, k)
    qh = rng.integers(-2, 3, size=(nq, dim)).astype(np.float32)
    ah = np.array([0.5, 0.0, 1.0, 0.5, 0.25, 0.75], np.float32)
    with sa.GpuIndex(segs) as ix:
        b = ix.prepare(offs_q, terms, w, k, sa.Wand)
        b.run()
        qv, a = _dev(torch, qh), _dev(torch, ah)
        outs = [torch.zeros((nq, k_out), dtype=torch.int32, device="cuda"),
                torch.zeros((nq, k_out), dtype=torch.int32, device="cuda"),
                torch.zeros((nq, k_out), dtype=torch.float32, device="cuda"),
                torch.zeros((nq, k_out), dtype=torch.float32, device="cuda"),
                torch.zeros((nq,), dtype=torch.int32, device="cuda")]
        b.rerank_device(1, qv.data_ptr(), a.data_ptr(), None, k_out, *[t.data_ptr() for t in outs])
        b.sync()
        b.close()
        got = [t.cpu().numpy() for t in outs]
    wd, ws, wsc, wc = want
    fields = [field]
    ed = np.zeros((nq, k_out), np.uint32)
    es = np.zeros((nq, k_out), np.uint32)
    esc = np.zeros((nq, k_out), np.float32)
    ec = np.zeros(nq, np.uint32)
    for i in range(nq):
        n = int(wc[i])
        q = dict(cf=[0], qv=[qh[i]], alpha=ah[i:i + 1], boost=None, seg=ws[i, :n], doc=wd[i, :n], bm=wsc[i, :n])
        d, s, sc, v = oracle_rerank_segments(oracle, fields, q, "one", k_out)
        m = len(d)
        ed[i, :m], es[i, :m], esc[i, :m], ec[i] = d, s, sc, m
        assert np.array_equal(got[3][i, :m], v), f"vec query {i}"
    assert_same_hits((got[0].view(np.uint32), got[1].view(np.uint32), got[2], got[4].view(np.uint32)),
                     (ed, es, esc, ec), what=f"batch rerank k_out {k_out}")


def test_batch_rerank_device_too_many_candidates():
    """A batch with k > 8192 (kRerankMaxCand) is a clean SLG_ERR_UNSUPPORTED for slg_batch_rerank_device."""
    import torch
    import searchlite_amd as sa
    from searchlite_amd import _native as N
    from tests.util import random_queries
    rng = np.random.default_rng(4)
    sg = random_segment(rng, 12000, 40, 8)
    sg.vec_dim, sg.vec_metric = 8, 0
    sg.vec_offsets = np.arange(sg.n_docs, dtype=np.uint32)
    sg.vec_values = np.ones((sg.n_docs, 8), np.float32)
    offs_q, terms, w = random_queries(rng, 2, 2, 40)
    with sa.GpuIndex([sg]) as ix:
        b = ix.prepare(offs_q, terms, w, 9000, sa.Wand)
        b.run()
        qv = torch.ones((2, 8), dtype=torch.float32, device="cuda")
        a = torch.full((2,), 0.5, dtype=torch.float32, device="cuda")
        o = [torch.zeros((2, 10), dtype=torch.int32, device="cuda") for _ in range(4)] + \
            [torch.zeros((2,), dtype=torch.int32, device="cuda")]
        with pytest.raises(N.SlgError) as e:
            b.rerank_device(1, qv.data_ptr(), a.data_ptr(), None, 10, *[t.data_ptr() for t in o])
        assert e.value.code == N.ERR_UNSUPPORTED
        b.sync()
        b.close()
