"""score_multi_kernel (searchlite_amd/csrc/slg_score_multi.hpp) at its chunk, slot, window and skip edges.

The worlds are those of tests/multi_worlds.py.  Every world runs at k on both sides of the top-k register widths, under
its strategies and under Bm25.  The batch is planned a second time on the CPU with the tuning and the champion tables
the index reports, which must give the device's slice and posting counts; on that plan the promised edges are checked
again (tests/test_multi_worlds.py) and tests/multi_model.py predicts the kernel's two exact counters.

Tolerance 0: the same (segment, doc) sequence and score bits as the oracle (its plan path for the plan worlds);
slg_stats.scored_docs of every query equals the docs the model's chunks hold, skip_counts() equals (the plan's
non-essential postings, the postings of the slots the model skips), and postings_advanced is the query's postings less
its skipped ones."""
import numpy as np
import pytest

from tests import multi_model as M
from tests import multi_worlds as MW
from tests.test_multi_worlds import WorldPlan, check_edges, check_model, plan_lib
from tests.util import assert_same_hits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return sa


@pytest.fixture(scope="module")
def lib():
    return plan_lib()


_want = {}


def oracle_rows(oracle, W, k):
    """the exhaustive top-k of the world's queries, computed once per (world, k)"""
    if (W.name, k) not in _want:
        _want[(W.name, k)] = oracle.search_batch(W.segs, W.offs, W.terms, W.w, k, strategy=oracle.BM25, **(W.plans or {}))
    return _want[(W.name, k)]


def distinct_docs(W):
    """docs of each query's lists, over the segments: what any unclassified run scores"""
    out = []
    for q in range(len(W.offs) - 1):
        n = 0
        for s, seg in enumerate(W.segs):
            ids = [int(t) for t in W.terms[int(W.offs[q]):int(W.offs[q + 1]), s] if t != MW.NO_TERM]
            n += len(np.unique(np.concatenate(M.lists_of(seg, ids))))
        out.append(n)
    return out


def run_and_check(b, P, want, what):
    """one run of prepared batch b against the oracle's rows and the counters of plan P -> (rows, counters)"""
    W = P.W
    b.run()
    got = b.fetch(want_stats=True)
    assert_same_hits(got[:4], want, 0.0, what)
    stats = got[4]
    scored = [int(stats[q].scored_docs) for q in range(P.nq)]
    advanced = [int(stats[q].postings_advanced) for q in range(P.nq)]
    counts = b.skip_counts()
    if P.facts.multi:
        assert scored == P.scored.tolist(), f"{what}: scored_docs {scored}, the model's chunks hold {P.scored.tolist()}"
        probed = int(P.facts.n_postings_nonessential) if P.block_skip else 0
        assert counts == (probed, int(P.skipped.sum())), f"{what}: skip_counts {counts}, model {(probed, int(P.skipped.sum()))}"
        assert advanced == (P.q_postings.astype(np.int64) - P.skipped).tolist(), f"{what}: postings_advanced {advanced}"
    else:   # (5..8 lists, unclassified: the few-term kernel scores every doc of the lists)
        assert scored == distinct_docs(W) and counts == (0, 0), f"{what}: scored_docs {scored}, skip_counts {counts}"
    return got[:4], (scored, advanced, counts)


@pytest.mark.parametrize("k", MW.ALL_KS)
@pytest.mark.parametrize("world", MW.WORLDS, ids=lambda f: f.__name__)
def test_world_rows_and_counters(gpu, oracle, lib, world, k):
    W = world()
    want = oracle_rows(oracle, W, k)
    with gpu.GpuIndex(W.segs, tuning=W.tuning) as ix:
        tune = ix.tuning()
        champs = [ix.champions(s) for s in range(len(W.segs))]
        for strategy in sorted(set(W.strategies) | {MW.BM25}):
            what = f"world {W.name} k={k} strategy={strategy}"
            P = WorldPlan(lib, W, k, strategy, tuning=tune, champs=champs)
            with ix.prepare(W.offs, W.terms, W.w, k, strategy, **(W.plans or {})) as b:
                info = b.info()
                assert (info["n_slices"], info["n_postings"]) == (P.facts.n_slices, P.facts.n_postings), \
                    f"{what}: the device plans {info}, the plan library {P.facts.n_slices} slices of {P.facts.n_postings}"
                check_edges(P)
                check_model(P)
                run_and_check(b, P, want, what)


@pytest.mark.parametrize("world", [MW.ms_probe_world, MW.plan_groups_world], ids=lambda f: f.__name__)
def test_a_second_run_of_the_batch_gives_the_same(gpu, oracle, lib, world):
    """the partition kernel zeroes the counters of a batch at every run: rows and counters repeat"""
    W = world()
    k = W.edge_ks[0]
    want = oracle_rows(oracle, W, k)
    with gpu.GpuIndex(W.segs, tuning=W.tuning) as ix:
        P = WorldPlan(lib, W, k, W.strategies[0], tuning=ix.tuning(), champs=[ix.champions(s) for s in range(len(W.segs))])
        with ix.prepare(W.offs, W.terms, W.w, k, W.strategies[0], **(W.plans or {})) as b:
            first = run_and_check(b, P, want, f"world {W.name}, first run")
            second = run_and_check(b, P, want, f"world {W.name}, second run")
    assert first[1] == second[1]
    for x, y in zip(first[0], second[0]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
