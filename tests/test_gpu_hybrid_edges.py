"""hy_gather_kernel (slg_hybrid.hpp) at its structural edges: every row-chunk instantiation of hy_score_rows at the
dimensions on both sides of its dispatch (256 / 260, 512 / 516, 768 / 772) with a partial last chunk, and workgroups
of two and four waves (spans of 128, 256 and 1024 candidate slots).

The worlds are tests/vector_edge_worlds.py; tests/test_vector_edge_worlds.py proves on the CPU the slot counts and
spans, the vector counts of the crafted 64-candidate batches, that the vectorised reference of the all-docs worlds
equals tests/hybrid_ref.py, and that at most 10 % of a case's queries are left out of the order check.  Tolerance
and order rule are test_gpu_hybrid's (TOL, GAP, its `check`)."""
import numpy as np
import pytest

from tests import hybrid_ref as R
from tests import vector_edge_worlds as E
from tests.test_gpu_hybrid import check

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def chunk_index(oracle):
    """the row-chunk world with one vector field per (dim, metric) case, added with add_vector_field"""
    import searchlite_amd as sa
    W = E.chunk_world()
    fields = [E.chunk_field(oracle, d, m) for d, m in E.CHUNK_CASES]
    with sa.GpuIndex(W.segs) as ix:
        for i, (stores, _) in enumerate(fields):
            assert ix.add_vector_field(stores) == i + 1
        yield ix, W, fields


@pytest.mark.parametrize("case", range(len(E.CHUNK_CASES)), ids=[f"dim{d}-m{m}" for d, m in E.CHUNK_CASES])
def test_row_chunk_edges(oracle, chunk_index, case):
    """hy_score_rows<1> (252, 256), <2> (260, 300, 512), <3> (516, 764, 768) and <0> (772), cosine and L2: all but
    256, 512 and 768 end inside a chunk of 256 floats, where lanes past the row's end are masked (L2 adds
    (a - a)^2).  The last four components of rows and queries are large (E.CHUNK_Q_TAIL).  Queries 0, 1 and 2 match
    one crafted list each, a single 64-candidate batch with 7, 1 and 61 docs that have a vector: groups of fewer
    than four rows."""
    ix, W, fields = chunk_index
    dim, metric = E.CHUNK_CASES[case]
    stores, qv = fields[case]
    all_fields = [W.field0] + [f[0] for f in fields]
    k, cand = E.CHUNK_K, E.CHUNK_CAND
    got = ix.search_hybrid(*W.qs, k, [case + 1], qv, E.CHUNK_ALPHA, cand, k)
    want = R.reference(oracle, W.segs, all_fields, [case + 1], *W.qs, k, qv, E.CHUNK_ALPHA, None, cand, k)
    assert all(w["gap"] >= E.GAP for w in want)   # (E.chunk_field redraws near-tie queries: nothing is skipped)
    check(got, want, k, 1, metric, f"dim {dim} metric {metric}")
    # the crafted queries: every matched doc is a BM25 hit or in the list; the lists hold 7, 1 and 61 -> 20 docs
    assert [len(want[q]["maps"][0]) for q in range(3)] == [7, 1, 20]
    assert [int(t) for t in got[5][:3]] == [want[q]["total"] for q in range(3)]


@pytest.mark.parametrize("span", sorted(E.WAVE_CASES))
def test_multi_wave_workgroups(oracle, span):
    """Workgroups of 2 (span 128) and 4 (spans 256, 1024) waves.  hy_run halves the span from 1024 while
    slots / span < 2048, so a launch of 262 144 / 524 288 / 2 097 152 candidate slots or more gets a span of
    128 / 256 / 1024; each world has at least 1.25 x its threshold and stays below the next.  The slots of a query
    are the lengths of its posting lists (here: 41 000 for the all-docs term, plus one word's list for two queries
    of three), so the regions differ in length, none of them a multiple of 64, and spans straddle query and segment
    boundaries at odd offsets.  The middle query has no term: an empty region between two
    full ones.  Every query's count, total and rows are checked (the vectorised reference takes milliseconds per
    query), all 70 of the span-1024 world included."""
    import searchlite_amd as sa
    W = E.wave_world()
    qs, qv, boost, want = E.wave_queries(oracle, span)
    nq = len(qv)
    slots = E.query_slots(W.text_segs, qs[0], qs[1])
    total = int(slots.sum())
    nxt = {128: 256, 256: 512, 1024: None}[span]
    assert total >= 1.25 * E.hy_threshold(span) and (nxt is None or total < E.hy_threshold(nxt))
    assert E.hy_span(total) == span and min(span, E.HY_THREADS) // 64 == (2 if span == 128 else 4)
    assert total * 8 <= 256 << 20    # one key range: the budget is a quarter of the pool's cap, at least 256 MiB
    assert slots[nq // 2] == 0 and slots[nq // 2 - 1] > 40_000 and slots[nq // 2 + 1] > 40_000
    assert len(set(slots.tolist())) > 3 and any(int(s) % 64 for s in slots)
    k, cand = E.WAVE_K, E.WAVE_CAND
    with sa.GpuIndex(W.text_segs) as ix:
        got = ix.search_hybrid(*qs, k, [0], qv, E.WAVE_ALPHA, cand, k, boost=boost)
    assert all(w["gap"] >= E.GAP for w in want)   # (E.wave_queries redraws near-tie queries: nothing is skipped)
    check(got, want, k, 1, 0, f"span {span}")
    for q, w in enumerate(want):  # (check asserts these too for every query it does not skip: here, all)
        assert int(got[5][q]) == w["total"] and int(got[4][q]) == min(k, w["total"])
    assert int(got[5][nq // 2]) == 0 and int(got[4][nq // 2]) == 0
