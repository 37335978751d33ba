"""tests/scan_ref.py against hand-derived cases: every rank_feature modifier on both sides of its branch,
reciprocal of 0, a doc without a value, a product that overflows, negative boost, the score of match_all and the
order of ties.  No device."""
import math

import numpy as np

from tests import scan_ref as R

F32 = np.float32
BELOW_M1, ABOVE_M1 = float(np.nextafter(-1.0, -2.0)), float(np.nextafter(-1.0, 0.0))
TINY = float(np.nextafter(0.0, 1.0))


def world_of(values, deleted=None, filters=None):
    """one segment, field 0 = `values` (one list per doc)"""
    n = len(values)
    return dict(n_docs=[n], deleted=[deleted], filters=filters or {}, fields={0: [values]})


def rf(**kw):
    return {"rank_feature": dict(field=0, **kw)}


def one(value, **kw):
    """the score of a single doc holding `value` (None: no value), or None when it is dropped"""
    s, kept, _ = R.scores(rf(**kw), world_of([[] if value is None else [value]]), 0)
    return F32(s[0]) if kept[0] else None


def test_modifier_branches_on_both_sides():
    # log: <= 0 gives 0, above it ln
    assert one(0.0, modifier="log") == F32(0.0)
    assert one(-3.0, modifier="log") == F32(0.0)
    assert one(TINY, modifier="log") == F32(math.log(TINY))
    assert one(math.e, modifier="log") == F32(1.0)
    # log1p: <= -1 gives 0 (ln_1p(-1) would be -inf), just above it a large negative number
    assert one(-1.0, modifier="log1p") == F32(0.0)
    assert one(BELOW_M1, modifier="log1p") == F32(0.0)
    assert one(ABOVE_M1, modifier="log1p") == F32(math.log1p(ABOVE_M1))
    assert one(0.0, modifier="log1p") == F32(0.0)
    assert one(1e-20, modifier="log1p") == F32(1e-20)  # (ln(1 + x) computed naively would be 0)
    # sqrt: < 0 gives 0; -0.0 is not < 0: sqrt(-0.0) = -0.0
    assert one(-4.0, modifier="sqrt") == F32(0.0)
    assert one(4.0, modifier="sqrt") == F32(2.0)
    assert np.signbit(one(-0.0, modifier="sqrt"))
    # reciprocal: == 0 gives 0 (both zeros), else 1 / x
    assert one(0.0, modifier="reciprocal") == F32(0.0) and not np.signbit(one(-0.0, modifier="reciprocal"))
    assert one(4.0, modifier="reciprocal") == F32(0.25)
    assert one(-0.5, modifier="reciprocal") == F32(-2.0)
    # none
    assert one(-7.5) == F32(-7.5) and one(-7.5, modifier="none") == F32(-7.5)


def test_missing_value_takes_missing_as_f32():
    assert one(None) == F32(0.0)  # (the default)
    assert one(None, missing=2.5, boost=2.0) == F32(5.0)
    # missing is an f32 before it is an f64: 0.1 -> 0.100000001490116...
    assert one(None, missing=0.1, modifier="reciprocal") == F32(1.0 / float(F32(0.1)))
    assert one(None, missing=-1.0, modifier="log1p") == F32(0.0)
    # only the FIRST value counts
    s, kept, _ = R.scores(rf(), world_of([[3.0, 100.0], [], [7.0]]), 0)
    assert s.tolist() == [3.0, 0.0, 7.0] and kept.all()


def test_non_finite_results_drop_the_doc():
    assert one(TINY, modifier="reciprocal") is None          # 1 / 5e-324 = inf: the modified value is not finite
    assert one(1e39) is None                                   # finite f64, inf as f32: the product is not finite
    assert one(3e38, boost=2.0) is None                        # the product overflows
    assert one(3e38, boost=1.0) == F32(3e38)
    assert one(1e39, boost=0.0) is None                        # inf * 0 = NaN
    assert one(1e39, modifier="log") == F32(math.log(1e39))    # the modifier brings it back
    assert one(1e-50) == F32(0.0)                               # an underflow is a finite score


def test_negative_boost_and_node_boost():
    assert one(2.0, boost=-1.5) == F32(-3.0)
    assert one(2.0, boost=-1.5, node_boost=2.0) == F32(-6.0)
    assert one(0.0, modifier="sqrt", boost=-1.0) == F32(-0.0) and np.signbit(one(0.0, modifier="sqrt", boost=-1.0))
    s, kept, _ = R.scores({"constant_score": {"boost": 0.1, "node_boost": 3.0}}, world_of([[], []]), 0)
    assert kept.all() and (s == F32(0.1) * F32(3.0)).all()
    # negative scores rank below positive ones, -0.0 below 0.0 (total_cmp)
    w = world_of([[1.0], [-1.0], [0.0], [-0.0]])
    (doc, seg, score, count), matched, _ = R.search([rf(boost=-1.0)], w, 4)
    assert doc[0].tolist() == [1, 3, 2, 0] and count[0] == 4 and matched[0] == 4
    assert score[0].view(np.uint32).tolist() == [F32(x).view(np.uint32) for x in (1.0, 0.0, -0.0, -1.0)]


def test_match_all_scores_one_and_counts_every_live_passing_doc():
    dead = np.array([0, 1, 0, 0, 0, 0], bool)
    w = dict(n_docs=[6, 3], deleted=[dead, None], fields={},
             filters={0: [np.array([1, 1, 1, 0, 1, 1], bool), None], 1: [np.array([1, 1, 0, 1, 1, 0], bool), np.zeros(3, bool)]})
    (doc, seg, score, count), matched, _ = R.search([{"match_all": {}}], w, 4)
    assert matched[0] == 8 and count[0] == 4
    assert list(zip(seg[0].tolist(), doc[0].tolist())) == [(0, 0), (0, 2), (0, 3), (0, 4)]  # ties: segment, then doc
    assert (score[0] == F32(1.0)).all()
    # node filter and root filter both apply, a None mask passes everything, rows past the count are zero
    q = [{"constant_score": {"filter": 0, "boost": 2.0}}]
    (doc, seg, score, count), matched, _ = R.search(q, w, 6, q_filter=np.array([1]))
    assert matched[0] == 2 and count[0] == 2 and doc[0].tolist() == [0, 4, 0, 0, 0, 0]
    assert score[0].tolist() == [2.0, 2.0, 0.0, 0.0, 0.0, 0.0]
    # k = 0 still counts
    (doc, _, _, count), matched, _ = R.search(q, w, 0)
    assert doc.shape == (1, 0) and count[0] == 0 and matched[0] == 7


def test_the_one_and_zero_rule_of_match_all_under_a_sort():
    """score order and a `_score` part: 1.0; a sort without `_score`: 0.0 (default_score).  constant_score and
    rank_feature keep their computed score there in the reference; the device reports 0.0 (the deviation)"""
    w = dict(n_docs=[3, 2], deleted=[np.array([0, 0, 1], bool), None], filters={}, fields={0: [[[4.0], [9.0], [1.0]], [[], [16.0]]]},
             sort_fields={"p": [[[5], [2, 7], [0]], [[], [2]]]})
    qs = [{"match_all": {}}, {"constant_score": {"boost": 2.5}}, rf(modifier="sqrt")]
    # asc: doc (0, 1) sorts by min(2, 7) = 2 and ties with (1, 1): segment breaks it; the doc without a value is last
    asc = R.search_sorted(qs, w, 10, [("p", "asc")])
    assert [r[:2] for r in asc[0][0]] == [(0, 1), (1, 1), (0, 0), (1, 0)] and asc[0][1] == 4
    assert [float(r[2]) for r in asc[0][0]] == [0.0] * 4                       # match_all: 0.0
    assert [float(r[2]) for r in asc[1][0]] == [2.5] * 4                       # constant_score: computed
    assert [float(r[2]) for r in asc[2][0]] == [3.0, 4.0, 2.0, 0.0]            # rank_feature: computed (missing 0)
    dev = R.search_sorted(qs, w, 10, [("p", "asc")], device=True)
    assert all(float(r[2]) == 0.0 for rows, _ in dev for r in rows)
    assert [[r[:2] for r in rows] for rows, _ in dev] == [[r[:2] for r in rows] for rows, _ in asc]
    # desc: (0, 1) sorts by max(2, 7) = 7; the doc without a value is still last
    desc = R.search_sorted(qs[:1], w, 3, [("p", "desc")])
    assert [r[:2] for r in desc[0][0]] == [(0, 1), (0, 0), (1, 1)] and desc[0][1] == 4
    # a `_score` part: match_all reports 1.0, on the device too
    for device in (False, True):
        sc = R.search_sorted(qs, w, 10, [("_score", "desc"), ("p", "asc")], device=device)
        assert [float(r[2]) for r in sc[0][0]] == [1.0] * 4
        assert [r[:2] for r in sc[2][0]] == [(1, 1), (0, 1), (0, 0), (1, 0)] and float(sc[2][0][0][2]) == 4.0
    (_, _, score, count), _, _ = R.search(qs[:1], w, 10)
    assert score[0, :count[0]].tolist() == [1.0] * 4                           # score order: 1.0


def test_order_of_ties_across_segments_and_drops_are_not_counted():
    w = dict(n_docs=[3, 3], deleted=[None, None], filters={},
             fields={0: [[[5.0], [1e39], [5.0]], [[7.0], [5.0], []]]})
    (doc, seg, score, count), matched, per_q = R.search([rf(missing=5.0)], w, 10)
    assert matched[0] == 5  # (the 1e39 doc is dropped: not counted)
    assert list(zip(seg[0, :5].tolist(), doc[0, :5].tolist())) == [(1, 0), (0, 0), (0, 2), (1, 1), (1, 2)]
    assert per_q[0][1].tolist() == [0, 2, 0, 1, 2]


def test_safe_tells_the_rounding_boundaries():
    mid = float(F32(1.0)) / 2 + float(np.nextafter(F32(1.0), F32(2.0))) / 2
    assert not R.safe(np.array([mid]))[0] and not R.safe(np.array([mid * (1 + 2.0 ** -45)]))[0]
    assert R.safe(np.array([mid * (1 + 2.0 ** -30)]))[0] and R.safe(np.array([1.0]))[0]
    w = world_of([[math.e], [2.0]])
    assert R.unsafe_docs([rf()], w) == set()  # (no transcendental function: nothing to be unsafe)
