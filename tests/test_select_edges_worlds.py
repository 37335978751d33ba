"""The CPU half of tests/test_gpu_select_edges.py: the worlds of tests/select_edge_worlds.py have the properties
the device cases rest on.  Candidate counts and ties come from the oracle, slice counts from the host planner
(lib/libslg_plan.so, as tests/test_plan.py reads them), the region pattern from tests/bool_ref.py."""
import numpy as np

from tests import bool_ref as B
from tests import select_edge_worlds as SW
from tests.test_gpu_cursor import ordered_rows
from tests.test_plan import RQ, Planned, default_tuning, lib  # noqa: F401  (lib: the planner library fixture)


def counts(oracle, W, names):
    return oracle.search_batch(W.segs, *W.queries(names), W.k_all, strategy=oracle.BM25)


def slices_per_query(lib, W, names, k, tuning):
    """RoundQuery.n_slices summed over each query's sub-queries (a bool, sorted or cursor batch plans at 1025)"""
    qs = W.queries(names)
    p = Planned(lib, W.segs, *qs, k, tuning=default_tuning(**tuning))
    assert p.h, p.err
    try:
        assert p.facts.cand_mode and p.facts.uniform
        sqs = p.array(0, RQ)
        out = np.zeros(len(names), np.int64)
        np.add.at(out, sqs["q"].astype(np.int64), sqs["n_slices"].astype(np.int64))
        refs = p.array(5, "<u4").reshape(-1, 2)   # the run of slices the select kernel walks
        assert (refs[:, 1] - refs[:, 0]).tolist() == out.tolist()
        return out.tolist(), sqs
    finally:
        p.close()


def test_last_range_cap_steps():
    assert [SW.last_range_cap(k, SW.SELECT_CAP) for k in SW.SMALL_KS] == [64, 64, 64, 128, 128, 256]
    assert SW.OVERSHOOT_NS == [64, 65, 128, 129, 256, 257, 513]
    assert [SW.last_range_cap(x, SW.SELECT_CAP) for x in (257, 1, 2049 - 2048, 2047, 2048)] == [512, 64, 64, 2048, 2048]
    assert SW.last_range_cap(1025 - 1024, SW.SORTED_CAP) == 64 and SW.last_range_cap(1023, SW.SORTED_CAP) == 1024
    assert SW.SWITCH_NS == (8192, 8193)


def test_range_counts(oracle, lib):
    """cases 1 and 2: every n of the matrix, one- and two-segment; the slice table holds every query"""
    W = SW.ranges_world()
    for names, ns, ks in ((W.topk_names, SW.TOPK_NS, SW.TOPK_KS), (W.sorted_names, SW.SORTED_NS, SW.SORTED_KS)):
        doc, seg, score, cnt = counts(oracle, W, names)
        assert cnt.tolist() == [n for n in ns for _ in "ab"]
        assert set(cnt.tolist()) >= {k + d for k in ks for d in (-1, 0, 1)} and max(cnt) > 1.4 * max(ks)
        for i, nm in enumerate(names):
            n_segs = len(set(seg[i, :cnt[i]].tolist()))
            assert n_segs == (1 if nm[0] == "a" else 2)
    for k in (2049, 1025):
        got, _ = slices_per_query(lib, W, W.topk_names, k, SW.NO_SEED)
        assert max(got) <= SW.MAX_SLICES and min(got) >= 1


def test_tie_structure(oracle):
    """case 3: one score bit pattern over both segments; the segment changes inside the first range and the doc id
    alone decides at every later boundary; the two-valued column changes at rank 1 024 (tie_x) / 1 025 (tie_y)"""
    W = SW.ties_world()
    names = ["tie_topk", "tie_x", "tie_y"]
    hits = counts(oracle, W, names)
    doc, seg, score, cnt = hits
    assert cnt.tolist() == [3 * SW.SELECT_CAP + 1, 3 * SW.SORTED_CAP + 1, 3 * SW.SORTED_CAP + 1]
    for q in range(3):
        assert len(set(score[q, :cnt[q]].view(np.uint32).tolist())) == 1
    cap = SW.SELECT_CAP
    assert seg[0, 0] != seg[0, cap - 1]
    for r in (cap, 2 * cap, 3 * cap):
        assert score[0, r - 1].view(np.uint32) == score[0, r].view(np.uint32) and seg[0, r - 1] == seg[0, r]
        assert doc[0, r - 1] < doc[0, r]
    cap = SW.SORTED_CAP
    rows = ordered_rows(hits, [("const", "asc")], W.fields)
    for q in (1, 2):
        assert rows[q][0].seg != rows[q][cap - 1].seg
        for r in (cap, 2 * cap, 3 * cap):
            assert rows[q][r - 1].values == rows[q][r].values == (7,) and rows[q][r - 1].seg == rows[q][r].seg
    rows = ordered_rows(hits, [("two", "asc"), ("_score", "desc")], W.fields)
    x, y = [h.values[0] for h in rows[1]], [h.values[0] for h in rows[2]]
    assert x[:cap] == [0] * cap and x[cap:] == [1] * (len(x) - cap)            # changes exactly at rank 1024
    assert y[:cap + 1] == [0] * (cap + 1) and y[cap + 1:] == [1] * (len(y) - cap - 1)   # at rank 1025
    assert rows[2][cap - 1].values == rows[2][cap].values                   # equal field parts across the boundary


def test_overshoot_counts(oracle, lib):
    """case 4: n = cap_last, cap_last + 1, 2 cap_last + 1 for every small k, all of one score; 8 192 and 8 193
    candidates in a slice table (n_flat is 0 in the strided form)"""
    W = SW.ties_world()
    names = [f"o{n}" for n in list(SW.OVERSHOOT_NS) + list(SW.SWITCH_NS)]
    doc, seg, score, cnt = counts(oracle, W, names)
    assert cnt.tolist() == list(SW.OVERSHOOT_NS) + list(SW.SWITCH_NS)
    for q in range(len(names)):
        assert len(set(score[q, :cnt[q]].view(np.uint32).tolist())) == 1
    for k in SW.SMALL_KS:
        cap_last = SW.last_range_cap(k, SW.SELECT_CAP)
        assert cap_last >= k and all(f"o{n}" in W.T for n in SW.overshoot_ns(k))
        assert SW.overshoot_ns(k) == (cap_last, cap_last + 1, 2 * cap_last + 1)
    got, _ = slices_per_query(lib, W, names, 1025, SW.NO_SEED)
    assert max(got) <= SW.MAX_SLICES
    for k in SW.SWITCH_KS:   # below the switch the final range sorts next_pow2(k) keys, above it kSelectCap
        assert SW.last_range_cap(k % SW.SELECT_CAP, SW.SELECT_CAP) < SW.SELECT_CAP


def test_slice_counts(oracle, lib):
    """case 5: 1, 2, 511, 512, 513 and 700 slices per query under the one-round-per-slice tuning, at every k the
    device runs them with"""
    W = SW.slices_world()
    names = list(SW.SLICE_QUERIES)
    for k in SW.SLICE_KS + (1025,):
        got, _ = slices_per_query(lib, W, names, k, SW.SLICE_TUNING)
        assert got == list(SW.SLICE_COUNTS)
    assert [c <= SW.MAX_SLICES for c in SW.SLICE_COUNTS] == [True, True, True, True, True, False, False]
    cnt = counts(oracle, W, names)[3]
    assert cnt.tolist() == [W.n[nm] for nm in names] == [30, 60, 96, 511 * 48, 512 * 48, 513 * 48, 700 * 48]


def test_region_pattern(lib):
    """case 5, empty slices: list E is 10 + 3 regions of 128 consecutive postings; the MUST list leaves
    REGION_SURVIVORS of them"""
    W = SW.slices_world()
    got, sqs = slices_per_query(lib, W, ["E", "E"], 1025, SW.REGION_TUNING)
    assert got == [13, 13]
    assert sqs["n_slices"].tolist() == [10, 3, 10, 3] and sqs["rounds_per_slice"].tolist() == [1] * 4
    assert sqs["n_rounds"].tolist() == [10, 3, 10, 3]   # the list is cut at strides of df / n_rounds = 128 postings
    masks = B.clause_masks(W.segs, SW.region_clauses(W))
    assert masks[1] is None
    for s, want in enumerate(SW.REGION_SURVIVORS):
        e = W.lists["E"][s]
        left = [int(masks[0][s][e[SW.REGION * j:SW.REGION * (j + 1)]].sum()) for j in range(len(want))]
        assert left == want
    flat = SW.REGION_SURVIVORS[0] + SW.REGION_SURVIVORS[1]
    assert flat[0] == 0 and flat[-1] == 0 and {1, 64} <= set(flat)
    assert any(a == 0 and b == 0 for a, b in zip(flat[1:-2], flat[2:-1]))   # two empty regions in a row, inside
    qs = W.queries(["E", "E"])
    assert B.scored_docs(W.segs, qs[0], qs[1], SW.region_clauses(W)).tolist() == [sum(flat), 128 * 13]
