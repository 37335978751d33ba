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


def hand_segment():
    """12 docs, three lists: A = docs 1, 4, 7; B = 4, 7, 9; C = 7"""
    from searchlite_amd.segment import Segment
    lists = [np.array([1, 4, 7], np.uint32), np.array([4, 7, 9], np.uint32), np.array([7], np.uint32)]
    tfs = [np.array([1, 2, 3], np.uint32), np.array([2, 1, 4], np.uint32), np.array([5], np.uint32)]
    return Segment(n_docs=12, term_offsets=np.array([0, 3, 6, 7], np.uint64), doc_ids=np.concatenate(lists),
                   tfs=np.concatenate(tfs), field_doc_len=[np.arange(5, 17).astype(F32)],
                   field_avgdl=np.array([10.5], F32), docs=12.0, k1=1.2, b=0.75)


def hand_impacts(oracle):
    """{list: {doc: impact}} of hand_segment, one score_tf call per posting"""
    imp = lambda tf, df, d: F32(oracle.score_tf(float(tf), float(df), float(5 + d), 10.5, 12.0, 1.2, 0.75, 1.0))
    return {"A": {1: imp(1, 3, 1), 4: imp(2, 3, 4), 7: imp(3, 3, 7)},
            "B": {4: imp(2, 3, 4), 7: imp(1, 3, 7), 9: imp(4, 3, 9)}, "C": {7: imp(5, 1, 7)}}


def one_query(terms, weights, **kw):
    n = len(terms)
    return dict(q_offsets=np.array([0, n], np.uint32), q_terms=np.array(terms, np.uint32).reshape(n, 1),
                q_weights=np.array(weights, F32), **kw)


def add(*xs):
    """f32 sum, left to right"""
    a = F32(xs[0])
    for x in xs[1:]:
        a = F32(a + F32(x))
    return a


def bits(m):
    return {k: int(np.asarray(v, F32).view(np.uint32)) for k, v in m.items()}


def test_direct_maps_leaf_and_term_order(oracle):
    """terms A, B, C, A on leaves 1, 0, 1, 0: leaf 0 = B w1 + A w3 (query-term order), leaf 1 = A w0 + C w2; a
    Sum adds leaf 0, then leaf 1, from -0.0; min_match 2 drops the docs one leaf holds"""
    I = hand_impacts(oracle)
    A, B, C = I["A"], I["B"], I["C"]
    w = [F32(x) for x in (0.7, 1.3, 2.9, 0.11)]
    z = F32(0.0)
    leaf0 = {1: add(z, A[1] * w[3]), 4: add(z, B[4] * w[1], A[4] * w[3]), 7: add(z, B[7] * w[1], A[7] * w[3]),
             9: add(z, B[9] * w[1])}
    leaf1 = {1: add(z, A[1] * w[0]), 4: add(z, A[4] * w[0]), 7: add(z, A[7] * w[0], C[7] * w[2])}
    want = {(0, d): add(F32(-0.0), leaf0[d], leaf1[d]) if d in leaf1 else add(F32(-0.0), leaf0[d]) for d in leaf0}
    rs = one_query([0, 1, 2, 0], w, q_leaf=np.array([1, 0, 1, 0], np.uint32))
    got = R.direct_maps(oracle, [hand_segment()], rs)[0]
    assert bits(got) == bits(want) and set(got) == {(0, 1), (0, 4), (0, 7), (0, 9)}
    got = R.direct_maps(oracle, [hand_segment()], dict(rs, q_min_match=2))[0]
    assert bits(got) == bits({k: v for k, v in want.items() if k != (0, 9)})
    # DisMax 0.3 over the same leaves: doc 9 has leaf 0 only, so 0.0 joins the max
    tie = F32(0.3)
    dm = {}
    for d in leaf0:
        ls = [leaf0[d]] + ([leaf1[d]] if d in leaf1 else [])
        m = max(ls + ([z] if len(ls) < 2 else []))
        dm[(0, d)] = F32(m + F32(tie * F32(add(z, *ls) - m)))
    got = R.direct_maps(oracle, [hand_segment()], dict(rs, q_plan=1, q_tie=tie))[0]
    assert bits(got) == bits(dm)


def test_direct_maps_negative_weights_and_overflow(oracle):
    I = hand_impacts(oracle)
    A, B = I["A"], I["B"]
    seg = hand_segment()
    # Sum of one negative leaf: -0.0 + x = x
    got = R.direct_maps(oracle, [seg], one_query([0], [-2.0]))[0]
    assert bits(got) == bits({(0, d): F32(A[d] * F32(-2.0)) for d in A})
    # DisMax 0.3, both leaves negative, q_nleaves 3 (a leaf nothing names): m = max(.., 0.0) = 0.0, r = 0.3 sum
    rs = one_query([0, 1], [-2.0, -0.5], q_plan=1, q_tie=F32(0.3), q_nleaves=3)
    got = R.direct_maps(oracle, [seg], rs)[0]
    a, b = F32(A[7] * F32(-2.0)), F32(B[7] * F32(-0.5))
    assert bits({(0, 7): got[(0, 7)]}) == bits({(0, 7): F32(F32(0.0) + F32(F32(0.3) * F32(F32(a + b) - F32(0.0))))})
    # with both leaves present and no third leaf: m = the larger (less negative) leaf
    got = R.direct_maps(oracle, [seg], dict(rs, q_nleaves=2))[0]
    m = max(a, b)
    assert bits({0: got[(0, 7)]}) == bits({0: F32(m + F32(F32(0.3) * F32(F32(a + b) - m)))})
    assert got[(0, 1)] == F32(F32(0.3) * F32(A[1] * F32(-2.0)))  # doc 1: leaf 1 is missing, m = 0.0
    # 3e38 and -3e38 on two leaves: inf + -inf = NaN; on one leaf alone: +inf
    with np.errstate(over="ignore", invalid="ignore"):
        got = R.direct_maps(oracle, [seg], one_query([0, 1], [3e38, -3e38]))[0]
        assert np.isnan(got[(0, 4)]) and np.isnan(got[(0, 7)])
        assert got[(0, 1)] == np.inf and got[(0, 9)] == -np.inf
        assert np.isnan(R.combine(R.TOTAL, 1.0, got[(0, 4)]))
        assert R.combine(R.MAX, 1.5, got[(0, 4)]) == F32(1.5) and R.combine(R.MIN, 1.5, got[(0, 4)]) == F32(1.5)
        assert R.combine(R.MULTIPLY, -1.5, got[(0, 1)]) == -np.inf


def test_total_order_of_nan_inf_and_zeros():
    """apply_rescore sorts by f32::total_cmp: +NaN > +inf > 1 > +0.0 > -0.0 > -1 > -inf > -NaN"""
    vals = [F32(-1.0), F32(np.inf), F32(0.0), F32(np.nan), F32(-np.inf), F32(-0.0), F32(1.0),
            np.array([0xFFC00000], np.uint32).view(F32)[0]]
    hits = [(0, i, 10.0 - i) for i in range(8)]
    with np.errstate(invalid="ignore"):
        out = R.apply_rescore(*rows(*hits), {(0, i): v for i, v in enumerate(vals)}, 8, R.MULTIPLY)
        want = [F32(F32(10.0 - i) * v) for i, v in enumerate(vals)]
    order = [3, 1, 6, 2, 5, 0, 4, 7]
    assert [int(d) for d in out[0]] == order
    assert out[2].view(np.uint32).tolist() == [int(np.asarray(want[i]).view(np.uint32)) for i in order]


def test_direct_maps_equal_the_exhaustive_run(oracle):
    """on ordinary queries (positive weights) both ways to r agree bit for bit, live docs"""
    from tests.util import random_queries, random_segment
    rng = np.random.default_rng(21)
    segs = [random_segment(rng, 120, 12, 6), random_segment(rng, 80, 12, 6)]
    segs[1].deleted = np.packbits(rng.random(80) < 0.2, bitorder="little")
    o, t, w = random_queries(rng, 6, 6, 12, n_segs=2, weights=True)
    t[5, 1] = t[9, 0] = 0xFFFFFFFF
    dead = np.unpackbits(segs[1].deleted, bitorder="little")
    for kw in ({}, dict(q_leaf=np.tile([1, 0, 1, 0, 1, 0], 6)),  # (three terms per leaf: the order of additions shows)
               dict(q_leaf=np.tile([0, 0, 0, 1, 1, 1], 6), q_plan=1, q_tie=F32(0.3)),
               dict(q_leaf=np.tile([0, 1, 1, 2, 2, 2], 6), q_plan=1, q_tie=F32(0.3), q_nleaves=4), dict(q_min_match=2),
               dict(q_leaf=np.tile([1, 0, 1, 0, 1, 0], 6), q_min_match=2)):
        rs = dict(q_offsets=o, q_terms=t, q_weights=w, **kw)
        a, b = R.rescore_maps(oracle, segs, rs), R.direct_maps(oracle, segs, rs)
        for q in range(6):
            live = {k: v for k, v in b[q].items() if not (k[0] == 1 and dead[k[1]])}
            assert bits(a[q]) == bits(live), (kw, q)
            assert len(live) > 0
