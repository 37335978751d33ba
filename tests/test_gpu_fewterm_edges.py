"""score_uniform4_kernel (searchlite_amd/csrc/slg_score_uni4.hpp) at its cut, lane, chunk, filter and join edges.

The worlds are those of tests/fewterm_worlds.py.  Every world runs at k on both sides of the top-k register widths, at
its own k values and at a k that shows every doc of every query, under each of its strategies, with the slices cut by
the scoring wave itself (inline_cuts 1) and by partition_rounds_kernel (inline_cuts 0).  The batch is planned a second
time on the CPU with the tuning and the champion tables the index reports, which must give the device's slice and
posting counts; on that plan the promised edges are checked again (tests/test_fewterm_worlds.py).

Tolerance 0: the same (segment, doc) sequence, score bits and counts as the oracle (its plan, filter and
minimum_should_match paths where the world has them); slg_stats.scored_docs of every query equals the distinct docs of
its lists (under min_match too: the matcher refuses a doc as a doc filter does, at the top-k insertion), postings_advanced its postings, skip_counts() is (0, 0); both ways of cutting give identical rows and
counters."""
import numpy as np
import pytest

from tests import fewterm_worlds as FW
from tests.test_fewterm_worlds import FewPlan, check_edges, check_model
from tests.test_multi_worlds import plan_lib
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
        plans = dict(W.plans or {})
        mm = plans.pop("q_min_match", None)
        if mm is not None:
            rows = oracle.search_batch_min_match(W.segs, W.offs, W.terms, W.w, k, mm, strategy=oracle.BM25, **plans)
        elif W.masks is not None:
            rows = oracle.search_batch_filtered(W.segs, W.offs, W.terms, W.w, k, np.zeros(W.nq, dtype=np.int32), [W.masks],
                                                strategy=oracle.BM25, **plans)
        else:
            rows = oracle.search_batch(W.segs, W.offs, W.terms, W.w, k, strategy=oracle.BM25, **plans)
        _want[(W.name, k)] = rows
    return _want[(W.name, k)]


def run_and_check(b, P, want, what):
    """one run of prepared batch b against the oracle's rows and the counters of plan P -> (rows, counters)"""
    b.run()
    got = b.fetch(want_stats=True)
    assert_same_hits(got[:4], want, 0.0, what)
    stats = got[4]
    scored = [int(stats[q].scored_docs) for q in range(P.nq)]
    advanced = [int(stats[q].postings_advanced) for q in range(P.nq)]
    counts = b.skip_counts()
    assert scored == P.docs.tolist(), f"{what}: scored_docs {scored}, the lists hold {P.docs.tolist()} distinct docs"
    assert advanced == P.postings.tolist(), f"{what}: postings_advanced {advanced}, the lists hold {P.postings.tolist()}"
    assert counts == (0, 0), f"{what}: skip_counts {counts}"
    return got[:4], (scored, advanced, counts)


def run_world(gpu, lib, W, k, strategy, inline_cuts, want, runs=1):
    with gpu.GpuIndex(W.segs, tuning=dict(W.tuning, inline_cuts=inline_cuts)) as ix:
        tune = ix.tuning()
        assert tune.inline_cuts == inline_cuts
        champs = [ix.champions(s) for s in range(len(W.segs))] if tune.champions else None
        fid = ix.add_filter(W.masks) if W.masks is not None else 0
        what = f"world {W.name} k={k} strategy={strategy} inline_cuts={inline_cuts}"
        P = FewPlan(lib, W, k, strategy, tuning=tune, champs=champs, filter_id=fid)
        qf = None if W.masks is None else np.full(W.nq, fid, dtype=np.int32)
        with ix.prepare(W.offs, W.terms, W.w, k, strategy, q_filter=qf, **(W.plans or {})) as b:
            info = b.info()
            assert (info["n_slices"], info["n_postings"]) == (P.facts.n_slices, P.facts.n_postings), \
                f"{what}: the device plans {info}, the plan library {P.facts.n_slices} slices of {P.facts.n_postings}"
            check_edges(P)
            check_model(P)
            return [run_and_check(b, P, want, f"{what} run {i}") for i in range(runs)]


MAX_KS = 9


@pytest.mark.parametrize("k_at", range(MAX_KS))
@pytest.mark.parametrize("world", FW.WORLDS, ids=lambda f: f.__name__)
def test_world_rows_and_counters(gpu, oracle, lib, world, k_at):
    """case k_at of a world runs its k_at-th k: ALL_KS, its own, the one that shows every doc.  The worlds are built when
    a case runs, not when the file is collected; a world with fewer k values has nothing left to run in its last cases."""
    W = world()
    assert len(W.ks) <= MAX_KS
    if k_at >= len(W.ks):
        return
    k = W.ks[k_at]
    want = oracle_rows(oracle, W, k)
    for strategy in W.strategies:
        (own,) = run_world(gpu, lib, W, k, strategy, 1, want)
        (parted,) = run_world(gpu, lib, W, k, strategy, 0, want)
        assert own[1] == parted[1], f"world {W.name} k={k}: counters differ between the two ways of cutting"
        for x, y in zip(own[0], parted[0]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"world {W.name} k={k}: rows differ"


@pytest.mark.parametrize("world", [FW.chunks4_world, FW.plans8_world], ids=lambda f: f.__name__)
def test_a_second_run_of_the_batch_gives_the_same(gpu, oracle, lib, world):
    """the partition kernel zeroes the counters of a batch at every run: rows and counters repeat"""
    W = world()
    k = W.full_k()
    first, second = run_world(gpu, lib, W, k, W.strategies[0], 1, oracle_rows(oracle, W, k), runs=2)
    assert first[1] == second[1]
    for x, y in zip(first[0], second[0]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
