"""The staging kernels of slg_stage.hpp (stage_impacts_kernel, stage_champions_kernel, filter_build_kernel,
posting_mark_kernel, bitmap_or_kernel) at their value, list-length and word edges, through what reads the state they
build: ordinary batches, GpuIndex.champions and GpuIndex.fetch_filter.

Tolerance 0: the same (segment, doc) sequence, score bits and counts as the oracle; every one-term score is the bit
pattern tests/stage_ref.impacts gives that posting; champion tables meet tests/stage_ref.check_champions and are bit
for bit those of a fresh index after an update; filter bitmaps equal tests/stage_ref.filter_pass.  The worlds are
those of tests/stage_worlds.py; tests/test_stage_worlds.py proves on the CPU that every edge named here is in them."""
import copy

import numpy as np
import pytest

from tests import stage_ref as R
from tests import stage_worlds as SW
from tests.util import assert_same_hits

pytestmark = pytest.mark.gpu

NO_TERM = SW.NO_TERM
bits = lambda a: np.asarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return sa


def strategies(sa):
    return (sa.Bm25, sa.Wand, sa.Bmw)


def only_segment(q_terms, s):
    """the same queries against segment s alone"""
    out = np.full_like(q_terms, NO_TERM)
    out[:, s] = q_terms[:, s]
    return out


# ---- impacts: world V ------------------------------------------------------------------------------------------
def check_one_term_scores(sa, oracle, ix, segs, s, what):
    """one-term queries of weight 1 over every non-empty list of segment s at k = n_docs: the oracle's rows, and
    every score the reference impact of its posting"""
    seg = segs[s]
    qo, qt, w = SW.v_queries(1)
    qt = only_segment(qt, s)
    want = oracle.search_batch(segs, qo, qt, w, seg.n_docs, strategy=oracle.BM25)
    imps = R.impacts(oracle, seg)
    dead = R.deleted_mask(seg)
    for strat in strategies(sa):
        got = ix.search_batch(qo, qt, w, seg.n_docs, strat)
        assert_same_hits(got, want, 0.0, f"{what} segment {s} strategy {strat}")
        doc, sg, score, count = got
        for q in range(len(count)):
            t = int(qt[qo[q], s])
            d, _ = seg.postings(t)
            n = int(count[q])
            assert n == int((~dead[d]).sum()), f"{what} segment {s} term {t}: {n} rows"
            assert (sg[q, :n] == s).all()
            at = int(seg.term_offsets[t]) + np.searchsorted(d, doc[q, :n])
            assert np.array_equal(seg.doc_ids[at], doc[q, :n])
            assert np.array_equal(bits(score[q, :n]), bits(imps[at])), f"{what} segment {s} term {t} strategy {strat}"


def check_multi_term(sa, oracle, ix, segs, what, strats=None):
    for n_terms in (3, 7):
        qo, qt, w = SW.v_queries(n_terms)
        want = oracle.search_batch(segs, qo, qt, w, SW.V_DOCS, strategy=oracle.BM25)
        for strat in strats or strategies(sa):
            assert_same_hits(ix.search_batch(qo, qt, w, SW.V_DOCS, strat), want, 0.0, f"{what} {n_terms} terms strategy {strat}")


def test_impacts_on_the_value_grid(gpu, oracle):
    segs = SW.v_segments()
    with gpu.GpuIndex([copy.copy(s) for s in segs]) as ix:
        for s in range(len(segs)):
            check_one_term_scores(gpu, oracle, ix, segs, s, "staged")
        check_multi_term(gpu, oracle, ix, segs, "staged")


@pytest.mark.parametrize("s", [0, 3])
def test_rederived_impacts_on_the_value_grid(gpu, oracle, s):
    """slg_index_update_deleted re-derives the impacts (doc ids read back from the padded layout) at the same edges:
    growing tombstones with doc 0 and the last doc, a live_docs below some df, then no bitmap and another live_docs"""
    segs = SW.v_segments()
    with gpu.GpuIndex([copy.copy(x) for x in segs]) as ix:
        for step, (deleted, live) in enumerate(SW.v_updates()):
            ix.update_deleted(s, deleted, live)
            segs[s] = SW.with_update(segs[s], deleted, live)
            what = f"update {step}"
            check_one_term_scores(gpu, oracle, ix, segs, s, what)
            check_multi_term(gpu, oracle, ix, segs, what)
            with gpu.GpuIndex([copy.copy(x) for x in segs]) as fresh:
                for n_terms in (1, 3, 7):
                    qo, qt, w = SW.v_queries(n_terms)
                    assert_same_hits(ix.search_batch(qo, qt, w, SW.V_DOCS, gpu.Wand),
                                     fresh.search_batch(qo, qt, w, SW.V_DOCS, gpu.Wand), 0.0, f"{what} vs a fresh index, {n_terms} terms")


# ---- impacts: world B ------------------------------------------------------------------------------------------
def test_more_postings_than_the_staging_grid_has_threads(gpu, oracle):
    """the staging kernel's grid-stride loop takes a second turn: the last list lies wholly in it"""
    seg = SW.b_segment()
    qo = np.array([0, 1, 2], dtype=np.uint32)
    qt = np.array([[0], [SW.B_LISTS - 1]], dtype=np.uint32)
    w = np.ones(2, dtype=np.float32)
    with gpu.GpuIndex([copy.copy(seg)]) as ix:
        for step in range(2):
            for k in (11, 300):
                want = oracle.search_batch([seg], qo, qt, w, k, strategy=oracle.BM25)
                for strat in strategies(gpu):
                    assert_same_hits(ix.search_batch(qo, qt, w, k, strat), want, 0.0, f"step {step} k {k} strategy {strat}")
            if step == 0:
                bm, live = SW.b_tombstones()
                ix.update_deleted(0, bm, live)
                seg = SW.with_update(seg, bm, live)


# ---- champions: world C ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cworld(gpu, oracle):
    seg = SW.c_segment()
    bm, live = SW.c_tombstones(seg)
    dead_seg = SW.with_update(seg, bm, live)
    base = gpu.GpuIndex([copy.copy(seg)])
    updated = gpu.GpuIndex([copy.copy(seg)])
    updated.update_deleted(0, bm, live)
    yield {"seg": seg, "dead_seg": dead_seg, "base": base, "updated": updated}
    base.close()
    updated.close()


def test_champion_table(gpu, oracle, cworld):
    seg = cworld["seg"]
    R.check_champions(cworld["base"].champions(0), seg, R.impacts(oracle, seg), "staged")


def test_champion_table_with_tombstones(gpu, oracle, cworld):
    seg = cworld["dead_seg"]
    imps = R.impacts(oracle, seg)
    with gpu.GpuIndex([copy.copy(seg)]) as fresh:
        table = fresh.champions(0)
    R.check_champions(table, seg, imps, "staged with tombstones")
    after = cworld["updated"].champions(0)
    assert np.array_equal(bits(after), bits(table)), "the table after update_deleted is not that of a fresh index"
    assert not np.array_equal(bits(after), bits(cworld["base"].champions(0)))


def test_champions_off_refuses(gpu):
    from searchlite_amd import _native as N
    with gpu.GpuIndex([SW.f_world()["segs"][3]], tuning={"champions": 0}) as ix:
        with pytest.raises(N.SlgError) as ei:
            ix.champions(0)
        assert ei.value.code == N.ERR_UNSUPPORTED and "champions" in ei.value.msg


def test_champions_of_a_segment_without_postings(gpu):
    from searchlite_amd.segment import Segment
    seg = Segment(n_docs=3, term_offsets=[0, 0, 0], doc_ids=[], tfs=[], field_doc_len=[np.ones(3)], field_avgdl=[1.0], docs=3.0)
    with gpu.GpuIndex([seg]) as ix:
        t = ix.champions(0)
    assert t.shape == (2, 68) and not t.any()


@pytest.mark.parametrize("k", SW.C_KS)
@pytest.mark.parametrize("which", ["base", "updated"])
def test_champion_seeds_and_bounds_lose_no_hit(gpu, oracle, cworld, which, k):
    """the table feeds the threshold seed (entry champ_index(k)) and MaxScore (entry 0): at every k on a boundary
    of champ_index, over lists whose k-th score lies exactly on the seed (all impacts equal)"""
    seg = cworld["seg" if which == "base" else "dead_seg"]
    for n_terms in (1, 3):
        qo, qt, w = SW.c_queries(n_terms)
        want = oracle.search_batch([seg], qo, qt, w, k, strategy=oracle.BM25)
        for strat in strategies(gpu):
            assert_same_hits(cworld[which].search_batch(qo, qt, w, k, strat), want, 0.0, f"{which} {n_terms} terms k {k} strategy {strat}")


# ---- the bitmap, range and term filters: world F ---------------------------------------------------------------
def register(ix, kind, args):
    if kind == "bitmap":
        return ix.add_filter(args)
    if kind in ("i64", "f64"):
        return ix.add_filter_range([a[0] for a in args], args[0][1], args[0][2])
    ids = np.array([a[0] for a in args], dtype=np.uint32).reshape(len(args), len(args[0][0])).T  # [n_terms, n_segs]
    masks = [a[2] for a in args]
    return ix.add_filter_terms(ids, pass_if_absent=args[0][1], and_masks=None if all(m is None for m in masks) else masks)


def check_filter(ix, fid, kind, args, segs, what):
    got = ix.fetch_filter(fid)
    for s, seg in enumerate(segs):
        want = R.filter_pass(kind, args[s], seg)
        assert np.array_equal(got[s], want), f"{what}: segment {s} ({seg.n_docs} docs), docs {np.nonzero(got[s] != want)[0][:8].tolist()} differ"


def test_filters_at_their_word_and_value_edges(gpu, oracle):
    W = SW.f_world()
    segs = list(W["segs"])
    cases = SW.f_cases(W)
    with gpu.GpuIndex([copy.copy(s) for s in segs]) as ix:
        ids = {}
        for name, kind, args in cases:
            ids[name] = register(ix, kind, args)
            check_filter(ix, ids[name], kind, args, segs, name)
        # new tombstones: every registered filter follows, and so does one registered afterwards
        for s, (bm, live) in SW.f_updates(W).items():
            ix.update_deleted(s, bm, live)
            segs[s] = SW.with_update(segs[s], bm, live)
        for name, kind, args in cases:
            check_filter(ix, ids[name], kind, args, segs, name + " after update_deleted")
        name, kind, args = cases[-1]
        check_filter(ix, register(ix, kind, args), kind, args, segs, name + " registered after update_deleted")
        # one batch with a filter of each kind
        pick = ["bitmap first", "i64 hi on a value", "f64 on the values", "terms absent and_masks", "terms present term 4"]
        by_name = {name: (kind, args) for name, kind, args in cases}
        qo = np.arange(len(pick) + 2, dtype=np.uint32)
        qt = np.tile(np.array(W["score_term"], dtype=np.uint32), (len(pick) + 1, 1))
        w = np.ones(len(pick) + 1, dtype=np.float32)
        q_filter = np.array([ids[p] for p in pick] + [-1], dtype=np.int32)
        masks = {ids[p]: [R.filter_pass(by_name[p][0], by_name[p][1][s], seg) for s, seg in enumerate(segs)] for p in pick}
        want = oracle.search_batch_filtered(segs, qo, qt, w, 50, q_filter, masks, strategy=oracle.BM25)
        assert want[3][1] > 0 and want[3][-1] == 50
        for strat in strategies(gpu):
            assert_same_hits(ix.search_batch(qo, qt, w, 50, strat, q_filter=q_filter), want, 0.0, f"filtered batch strategy {strat}")
