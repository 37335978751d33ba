"""tests/hybrid_ref.py (the numpy restatement the GPU hybrid tests compare against) on hand-derived cases of
merge_vector_hits / compute_hybrid_score (api/reader.rs:225-254, :2474-2537)."""
import numpy as np

from tests import hybrid_ref as R

F32 = np.float32


def test_doc_outside_the_bm25_hits_scores_with_bm25_zero():
    # doc (0, 5) matches the text (it is in the clause list) but is not among the BM25 hits: bm25 = 0.0
    hits = [(0, 1, 4.0), (0, 2, 3.0)]
    maps = [{(0, 5): F32(0.5), (0, 1): F32(0.25)}]
    rows, total, _ = R.merge_vector_hits(hits, maps, [0.5], [0], 10)
    assert total == 3
    got = {(s, d): (f, v) for s, d, f, v in rows}
    assert got[(0, 5)] == (F32(0.25), F32(0.5))          # 0.5 * 0 + 0.5 * 0.5
    assert got[(0, 1)] == (F32(2.125), F32(0.25))        # 0.5 * 4 + 0.5 * 0.25
    assert got[(0, 2)] == (F32(1.0), None)               # 0.5 * 3 + 0.5 * -1 (missing, cosine)
    assert [r[:2] for r in rows] == [(0, 1), (0, 2), (0, 5)]


def test_alpha_zero_one_and_mixed():
    hits = [(0, 1, 2.0)]
    maps = [{(0, 1): F32(0.5)}, {(0, 1): F32(-0.25)}, {(0, 1): F32(1.0)}]
    rows, total, _ = R.merge_vector_hits(hits, maps, [0.0, 1.0, 0.25], [0, 0, 0], 5)
    # clause 0: vec 0.5; clause 1: bm25 2.0; clause 2: 0.25 * 2 + 0.75 * 1 = 1.25; mean = 3.75 / 3
    assert total == 1 and rows[0][2] == F32(F32(3.75) / F32(3.0)) and rows[0][3] == F32(1.25)
    # alpha = 1 everywhere: the final score is the BM25 score, docs found by vectors only score 0
    rows, total, _ = R.merge_vector_hits(hits, [{(1, 0): F32(0.9)}], [1.0], [0], 5)
    assert [(r[0], r[1], r[2]) for r in rows] == [(0, 1, F32(2.0)), (1, 0, F32(0.0))]


def test_all_vector_only_drops_docs_without_a_vector():
    hits = [(0, 1, 9.0), (0, 2, 8.0)]
    maps = [{(0, 2): F32(0.5)}, {(0, 3): F32(0.1)}]
    rows, total, _ = R.merge_vector_hits(hits, maps, [0.0, -1.0], [0, 0], 10)
    assert total == 2 and [r[:2] for r in rows] == [(0, 2), (0, 3)]   # (0, 1) is in no list: dropped
    assert rows[0][2] == F32(F32(0.5) + F32(-1.0)) / F32(2.0)
    # one clause with alpha > 0: nothing is dropped
    rows, total, _ = R.merge_vector_hits(hits, maps, [0.0, 0.5], [0, 0], 10)
    assert total == 3 and any(r[:2] == (0, 1) and r[3] is None for r in rows)


def test_missing_vector_score_per_metric():
    hits = [(0, 1, 1.0)]
    rows, _, _ = R.merge_vector_hits(hits, [{(0, 9): F32(0.0)}], [0.5], [0], 5)
    assert {r[:2]: r[2] for r in rows}[(0, 1)] == F32(0.0)           # 0.5 * 1 + 0.5 * -1.0
    rows, _, _ = R.merge_vector_hits(hits, [{(0, 9): F32(-2.0)}], [0.5], [1], 5)
    assert {r[:2]: r[2] for r in rows}[(0, 1)] == F32(F32(0.5) + F32(F32(0.5) * R.F32_MIN))
    assert R.missing(0) == F32(-1.0) and R.missing(1) == F32(np.finfo(np.float32).min)


def test_exact_ties_in_segment_doc_order_and_truncation():
    ents = [(F32(0.5), 1, 0), (F32(0.5), 0, 7), (F32(0.5), 0, 3), (F32(0.75), 2, 2), (F32(0.1), 0, 0)]
    m, gap = R.clause_list(ents, 3)
    assert set(m) == {(2, 2), (0, 3), (0, 7)} and gap == 0.0        # the tie is cut in (segment, doc) order
    m, gap = R.clause_list(ents, 4)
    assert set(m) == {(2, 2), (0, 3), (0, 7), (1, 0)} and abs(gap - 0.4) < 1e-6
    m, gap = R.clause_list(ents, 9)
    assert len(m) == 5 and gap == np.inf
    maps = [{(1, 4): F32(0.5), (0, 9): F32(0.5), (0, 2): F32(0.5)}]
    rows, total, gap = R.merge_vector_hits([], maps, [0.0], [0], 2)
    assert [r[:2] for r in rows] == [(0, 2), (0, 9)] and total == 3 and gap == 0.0


def test_boundary_keys_name_the_docs_of_a_near_tie():
    ents = [(F32(0.9), 0, 0), (F32(0.50001), 0, 1), (F32(0.5), 0, 2), (F32(0.49999), 0, 3), (F32(0.1), 0, 4)]
    assert R.boundary_keys(ents, 2) == {(0, 1), (0, 2), (0, 3)}   # 0.49999 is within 4e-5 of the cut's low score
    assert R.boundary_keys(ents, 1) == {(0, 0), (0, 1), (0, 2), (0, 3)}   # 0.50001 - 4e-5 < 0.49999
    assert R.boundary_keys(ents[:1] + ents[3:], 1) == {(0, 0), (0, 3)}    # a wide gap: the two docs at the cut
    assert R.boundary_keys(ents, 4) == {(0, 1), (0, 2), (0, 3), (0, 4)}
    assert R.boundary_keys(ents, 5) == set() and R.boundary_keys(ents, 0) == set()


def test_total_cmp_orders_negative_zero_below_zero():
    assert R.tkey(F32(-0.0)) < R.tkey(F32(0.0)) < R.tkey(F32(1e-30))
    # a blended sum starts at +0.0, so a lone -0.0 blend becomes +0.0 (api/reader.rs:232,249)
    rows, _, _ = R.merge_vector_hits([], [{(0, 1): F32(-0.0)}], [0.0], [0], 1)
    assert rows[0][2].tobytes() == F32(0.0).tobytes()
