"""tests/rescore_ref.py against hand-derived cases on a dozen docs (the reference of tests/test_gpu_rescore.py
must itself be right): every score mode, an unmatched row kept under multiply, a window smaller than the row
count leaving the tail in place, exact ties by segment then doc.  One case runs the whole chain over the
oracle on a hand-built segment."""
import numpy as np
import pytest

from tests import rescore_ref as R

F32 = np.float32


def rows(*hits, k=None):
    """hits (seg, doc, score) -> first-pass rows padded to k"""
    k = k or len(hits)
    doc, seg, score = np.zeros(k, np.uint32), np.zeros(k, np.uint32), np.zeros(k, F32)
    for i, (s, d, v) in enumerate(hits):
        seg[i], doc[i], score[i] = s, d, v
    return doc, seg, score, len(hits)


def as_hits(out, n):
    doc, seg, score = out[:3]
    return [(int(seg[i]), int(doc[i]), float(score[i])) for i in range(n)]


HITS = [(0, 3, 8.0), (0, 5, 6.0), (1, 2, 4.0), (0, 9, 2.0), (1, 7, 1.0)]
RMAP = {(0, 5): F32(3.0), (1, 2): F32(0.5), (1, 7): F32(10.0), (0, 11): F32(99.0)}  # (0, 11) is no row


@pytest.mark.parametrize("mode,want", [
    (R.TOTAL, [(1, 7, 11.0), (0, 5, 9.0), (0, 3, 8.0), (1, 2, 4.5), (0, 9, 2.0)]),
    (R.SUM, [(1, 7, 11.0), (0, 5, 9.0), (0, 3, 8.0), (1, 2, 4.5), (0, 9, 2.0)]),
    (R.MULTIPLY, [(0, 5, 18.0), (1, 7, 10.0), (0, 3, 8.0), (0, 9, 2.0), (1, 2, 2.0)]),
    (R.MAX, [(1, 7, 10.0), (0, 3, 8.0), (0, 5, 6.0), (1, 2, 4.0), (0, 9, 2.0)]),
    (R.MIN, [(0, 3, 8.0), (0, 5, 3.0), (0, 9, 2.0), (1, 7, 1.0), (1, 2, 0.5)]),
])
def test_every_mode(mode, want):
    out = R.apply_rescore(*rows(*HITS, k=7), RMAP, 5, mode)
    assert as_hits(out, 5) == want
    doc, seg, score, first, rsc, flag = out
    assert np.all(doc[5:] == 0) and np.all(score[5:] == 0) and np.all(flag[5:] == 0)
    # the detail arrays travel with their rows
    for i in range(5):
        key = (int(seg[i]), int(doc[i]))
        assert float(first[i]) == dict(((s, d), v) for s, d, v in HITS)[key]
        assert int(flag[i]) == (1 if key in RMAP else 0)
        assert float(rsc[i]) == float(RMAP.get(key, 0.0))


def test_unmatched_row_is_kept_under_multiply():
    """rows the rescore query does not match are neither multiplied by 0 nor removed"""
    out = R.apply_rescore(*rows(*HITS), {(0, 5): F32(0.0)}, 5, R.MULTIPLY)
    assert as_hits(out, 5) == [(0, 3, 8.0), (1, 2, 4.0), (0, 9, 2.0), (1, 7, 1.0), (0, 5, 0.0)]
    assert list(out[5]) == [0, 0, 0, 0, 1]


def test_window_smaller_than_count_leaves_the_tail_in_place():
    """only hits[..window] is sorted: a window row may end below the rows behind the window"""
    out = R.apply_rescore(*rows(*HITS), {(0, 3): F32(-7.5), (1, 7): F32(100.0)}, 2, R.TOTAL)
    assert as_hits(out, 5) == [(0, 5, 6.0), (0, 3, 0.5), (1, 2, 4.0), (0, 9, 2.0), (1, 7, 1.0)]
    assert list(out[5]) == [0, 1, 0, 0, 0]  # (1, 7) lies behind the window: not rescored
    assert [float(x) for x in out[3]] == [6.0, 8.0, 4.0, 2.0, 1.0]


def test_exact_ties_by_segment_then_doc():
    hits = [(1, 4, 5.0), (0, 9, 4.0), (1, 1, 3.0), (0, 2, 2.0), (0, 6, 1.0)]
    rmap = {(1, 4): F32(0.0), (0, 9): F32(0.0), (1, 1): F32(0.0), (0, 2): F32(0.0)}
    out = R.apply_rescore(*rows(*hits), rmap, 5, R.MULTIPLY)
    assert as_hits(out, 5) == [(0, 6, 1.0), (0, 2, 0.0), (0, 9, 0.0), (1, 1, 0.0), (1, 4, 0.0)]


def test_empty_cases():
    base = rows(*HITS)
    for rmap, window in ((RMAP, 0), ({}, 5), (None, 5)):
        out = R.apply_rescore(*base, rmap, window, R.TOTAL)
        assert as_hits(out, 5) == [(s, d, v) for s, d, v in HITS] and not out[5].any() and not out[4].any()
    out = R.apply_rescore(*rows(k=3), RMAP, 3, R.TOTAL)  # no row at all
    assert not out[2].any() and not out[5].any()
    out = R.apply_rescore(*base, RMAP, 5000, R.TOTAL)  # a window beyond the rows is capped at the count
    assert as_hits(out, 5)[0] == (1, 7, 11.0)


def test_total_order_of_signed_zeros():
    """-0.0 sorts below +0.0 (f32::total_cmp), as in the first pass"""
    hits = [(0, 1, 2.0), (0, 2, 1.0)]
    out = R.apply_rescore(*rows(*hits), {(0, 1): F32(-0.0), (0, 2): F32(0.0)}, 2, R.MULTIPLY)
    assert as_hits(out, 2)[0][:2] == (0, 2) and np.signbit(out[2][1])


def test_chain_over_the_oracle(oracle):
    """A hand-built segment of 12 docs: the rescore term's list holds docs 1, 4 and 7; r of a doc is the
    oracle's score_tf at the rescore weight, and the rows move as computed by hand."""
    from searchlite_amd.segment import Segment
    n = 12
    lists = [np.arange(n, dtype=np.uint32), np.array([1, 4, 7], np.uint32)]
    tfs = [np.arange(n, 0, -1).astype(np.uint32), np.array([1, 2, 3], np.uint32)]  # first pass: doc 0 best
    seg = Segment(n_docs=n, term_offsets=np.array([0, n, n + 3], np.uint64), doc_ids=np.concatenate(lists),
                  tfs=np.concatenate(tfs), field_doc_len=[np.full(n, 10.0, F32)],
                  field_avgdl=np.array([10.0], F32), docs=float(n), k1=1.2, b=0.75)
    qs = (np.array([0, 1], np.uint32), np.array([[0]], np.uint32), np.array([1.0], F32))
    rescore = dict(q_offsets=np.array([0, 1], np.uint32), q_terms=np.array([[1]], np.uint32),
                   q_weights=np.array([2.0], F32), window=8, mode=R.TOTAL)
    doc, sg, score, count, first, rsc, flag = R.reference(oracle, [seg], *qs, 10, rescore)
    fd, _, fs, fc = oracle.search_batch([seg], *qs, 10)
    assert list(fd[0]) == list(range(10)) and int(count[0]) == int(fc[0]) == 10
    r = {d: F32(oracle.score_tf(float(tf), 3.0, 10.0, 10.0, float(n), 1.2, 0.75, 2.0)) for d, tf in zip((1, 4, 7), (1, 2, 3))}
    want = sorted(((F32(fs[0, i] + r[i]) if i in r else fs[0, i], i) for i in range(8)), key=lambda e: (-e[0], e[1]))
    assert [int(d) for d in doc[0, :8]] == [d for _, d in want]
    assert [float(x) for x in score[0, :8]] == [float(v) for v, _ in want]
    assert list(doc[0, 8:]) == [8, 9] and list(flag[0, 8:]) == [0, 0]
    for i in range(8):
        d = int(doc[0, i])
        assert int(flag[0, i]) == (1 if d in r else 0) and float(rsc[0, i]) == float(r.get(d, 0.0))
        assert float(first[0, i]) == float(fs[0, d])
