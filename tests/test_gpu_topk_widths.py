"""Every top-k register width at its k boundaries.

The scoring kernels (score_uniform4_kernel kinds 6-9, score_multi_kernel MODE 0-4), their buffered top-k
(BufTopK: 64 * (KREGS + 1) LDS entries), merge_topk_kernel and merge_shards_kernel are compiled once per
register width KREGS = 1 / 2 / 4 / 8 / 16, picked from k (<= 64 / 128 / 256 / 512 / more).  Each family of
tests.util.topk_family (tests/test_plan.py proves which instantiation it reaches) runs at k on both sides of
every boundary, under the default tuning and under one without a threshold seed and with one round per
slice; bit-exact against the oracle.  The shard merge is checked directly against a numpy lexsort.
"""
import numpy as np
import pytest

from tests.util import TOPK_FAMILIES, TOPK_WIDTH_KS, assert_same_hits, random_segment, topk_family, topk_variants

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return sa


_families, _wants = {}, {}


def _family(name):
    if name not in _families:
        _families[name] = topk_family(name)
    return _families[name]


def _want(oracle, name, k):
    """Oracle result of family `name` at k (the same for both tuning variants); the data properties the
    matrix relies on are checked here, once (the tie across the cut on the oracle's top k + 1)."""
    if (name, k) not in _wants:
        from tests.util import TOPK_BOUNDARY_DFS, TOPK_FEW_DFS
        fam = _family(name)
        run = lambda kk: oracle.search_batch_filtered(fam["segs"], fam["offs"], fam["terms"], fam["w"], kk,
                                                      fam["q_filter"], [fam["masks"]], strategy=oracle.BM25,
                                                      **fam["plans"])
        want, top = run(k), run(k + 1)
        cnt = want[3].astype(np.int64)
        assert cnt[3] == 0                                   # no term anywhere
        assert cnt[5:7].tolist() == [min(df, k) for df in TOPK_FEW_DFS]
        assert (cnt == k).any(), (name, k, sorted(cnt.tolist()))
        if k >= 64:                                          # some query matches, but fewer than k docs
            assert ((cnt > 0) & (cnt < k)).any(), (name, k, sorted(cnt.tolist()))
        if name in ("F1", "F5"):                             # the crafted lists: live df exactly 64 .. 1025
            assert cnt[8:16].tolist() == [min(df, k) for df in TOPK_BOUNDARY_DFS]
        # an exact tie across the cut inside one segment: only the doc id decides what is kept
        full = top[3] > k
        cut = full & (top[2][:, k - 1].view(np.uint32) == top[2][:, k].view(np.uint32)) & (top[1][:, k - 1] == top[1][:, k])
        assert cut.any(), (name, k)
        _wants[(name, k)] = want
    return _wants[(name, k)]


@pytest.mark.parametrize("variant", ["a", "b"])
@pytest.mark.parametrize("name", TOPK_FAMILIES)
def test_topk_width_matrix(gpu, oracle, name, variant):
    """One index per (family, tuning variant), one batch at every k of TOPK_WIDTH_KS: identical
    (segment, doc) sequences, bit-identical scores and equal counts.  Two segments, tombstones among the
    top scorers, a doc filter on a third of the queries, exact score ties at the k-th place."""
    fam = _family(name)
    tuning = dict(fam["tuning"], **topk_variants(name)[variant])
    with gpu.GpuIndex(fam["segs"], tuning=tuning) as ix:
        fid = ix.add_filter(fam["masks"])
        qf = np.where(fam["q_filter"] >= 0, fid, -1).astype(np.int32)
        for k in TOPK_WIDTH_KS:
            want = _want(oracle, name, k)
            got = ix.search_plan(fam["offs"], fam["terms"], fam["w"], k, strategy=fam["strategy"], q_filter=qf,
                                 **fam["plans"])
            assert_same_hits(got, want, 0.0, f"{name} variant {variant} k={k}")


# ---- slg_merge_shards_device against a numpy reference ----------------------------------------------
_SCORES = np.array([-3.0, -1.5, -0.0, 0.0, 0.25, 1.0, 2.0, 7.5], dtype=np.float32)


def _total_key(score):
    """f32::total_cmp order as an int64 key (-0.0 below +0.0)."""
    b = np.asarray(score, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, b ^ 0x7FFFFFFF, b)


def _shard_rows(rng, n_shards, nq, k, seg_stride):
    """[n_shards, nq, k] doc / seg / score rows and [n_shards, nq] counts, each row sorted by (score desc,
    seg asc, doc asc) with unique (seg, doc); counts cover 0, 1, < k and exactly k, never above k."""
    doc = np.zeros((n_shards, nq, k), np.uint32)
    seg = np.zeros((n_shards, nq, k), np.uint32)
    score = np.zeros((n_shards, nq, k), np.float32)
    cnt = np.zeros((n_shards, nq), np.uint32)
    n_seg = seg_stride   # local segments 0 .. seg_stride-1: global segment = shard * stride + seg is unique
    for sh in range(n_shards):
        for q in range(nq):
            n = [0, 1, k, max(1, k // 2), k, int(rng.integers(0, k + 1))][(sh + q) % 6]
            x = rng.choice(3 * k * n_seg + 8, size=n, replace=False)
            sc = rng.choice(_SCORES, size=n)
            s_, d_ = (x % n_seg).astype(np.uint32), (x // n_seg).astype(np.uint32)
            o = np.lexsort((d_, s_, -_total_key(sc)))
            doc[sh, q, :n], seg[sh, q, :n], score[sh, q, :n] = d_[o], s_[o], sc[o]
            doc[sh, q, n:], seg[sh, q, n:], score[sh, q, n:] = 0xDEAD, 0xBEEF, np.float32(-9.0)  # never read
            cnt[sh, q] = n
    return doc, seg, score, cnt


def _merge_reference(doc, seg, score, cnt, k, seg_stride):
    n_shards, nq, _ = doc.shape
    out = (np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.float32),
           np.zeros(nq, np.uint32))
    for q in range(nq):
        d = np.concatenate([doc[sh, q, :cnt[sh, q]] for sh in range(n_shards)]).astype(np.int64)
        g = np.concatenate([sh * seg_stride + seg[sh, q, :cnt[sh, q]].astype(np.int64) for sh in range(n_shards)])
        sc = np.concatenate([score[sh, q, :cnt[sh, q]] for sh in range(n_shards)])
        o = np.lexsort((d, g, -_total_key(sc)))[:k]
        n = len(o)
        out[0][q, :n], out[1][q, :n], out[2][q, :n], out[3][q] = d[o], g[o], sc[o], n
    return out


@pytest.mark.parametrize("n_shards", [1, 3, 8])
def test_merge_shards_device_every_width(gpu, n_shards):
    """merge_shards_kernel<1/2/4/8/16> and merge_shards_large_kernel (k > 1024) on synthetic shard rows:
    the global top-k by (score desc by total_cmp, shard * seg_stride + seg asc, doc asc), every score and
    its sign bit exact, and slots past the count padded with doc 0, seg 0, score +0.0.  Scores come from a
    small set with negatives and both zeros, so most ranks are decided across shards by the tie-break."""
    import torch
    rng = np.random.default_rng(700 + n_shards)
    nq = 6
    with gpu.GpuIndex([random_segment(rng, 64, 4, 4)]) as ix:
        ix.set_stream(torch.cuda.current_stream().cuda_stream)
        for seg_stride in (1, 4):
            for k in (1, 63, 64, 65, 128, 129, 255, 256, 257, 512, 513, 1000, 1024, 1025):
                doc, seg, score, cnt = _shard_rows(rng, n_shards, nq, k, seg_stride)
                want = _merge_reference(doc, seg, score, cnt, k, seg_stride)
                dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
                g_doc, g_seg, g_score, g_cnt = dev(doc), dev(seg), dev(score), dev(cnt)
                m_doc = torch.full((nq, k), 0x5A5A, dtype=torch.int32, device="cuda")   # padding must be written
                m_seg = torch.full((nq, k), 0x5A5A, dtype=torch.int32, device="cuda")
                m_score = torch.full((nq, k), -5.0, dtype=torch.float32, device="cuda")
                m_cnt = torch.full((nq,), 0x7777, dtype=torch.int32, device="cuda")
                ix.merge_shards_device(n_shards, nq, k, g_doc.data_ptr(), g_seg.data_ptr(), g_score.data_ptr(),
                                       g_cnt.data_ptr(), seg_stride, m_doc.data_ptr(), m_seg.data_ptr(),
                                       m_score.data_ptr(), m_cnt.data_ptr())
                torch.cuda.synchronize()
                got = (m_doc.cpu().numpy().view(np.uint32), m_seg.cpu().numpy().view(np.uint32),
                       m_score.cpu().numpy(), m_cnt.cpu().numpy().view(np.uint32))
                what = f"{n_shards} shards, k={k}, seg_stride={seg_stride}"
                assert np.array_equal(got[3], want[3]), what
                assert np.array_equal(got[0], want[0]), what
                assert np.array_equal(got[1], want[1]), what
                assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), what   # padding: +0.0 bits
