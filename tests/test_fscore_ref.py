"""Hand-derived cases for tests/fscore_ref.py, the numpy restatement of function_score the GPU tests compare with:
every kind, every modifier on both sides of its branch, every score mode and boost mode, the effective-base rule,
the order max_boost -> min_score -> boost, "no present value", and the rounding guard."""
import math
import types

import numpy as np
import pytest

from tests import fscore_ref as R

F32 = np.float32


def world():
    """one segment of 6 docs; column 0 (f64): 4.0 | -1.0, 9.0 | none | 0.0 | -3.0 | 1e308; column 1 (i64): doc d has
    10 * d, doc 2 none; filter 0 passes docs 0, 1, 2; doc 5 is tombstoned"""
    seg = types.SimpleNamespace(n_docs=6, deleted=np.packbits(np.arange(6) == 5, bitorder="little"))
    f64 = [[4.0], [-1.0, 9.0], [], [0.0], [-3.0], [1e308]]
    i64 = [[10 * d] if d != 2 else [] for d in range(6)]
    return R.Columns([seg], {0: ([f64], np.float64), 1: ([i64], np.int64)}, {0: [np.arange(6) < 3]})


DOCS = np.arange(6)


def value(fn):
    val, has, _ = R.function_value(fn, world(), 0, DOCS)
    return [float(v) if h else None for v, h in zip(val, has)]


def test_weight_and_its_filter():
    assert value(dict(kind="weight", weight=2.5)) == [2.5] * 6
    assert value(dict(kind="weight", weight=2.5, filter=0)) == [2.5, 2.5, 2.5, None, None, None]


def test_field_value_factor_first_value_missing_and_overflow():
    fvf = lambda **kw: dict(kind="field_value_factor", field=0, **kw)
    assert value(fvf())[:5] == [4.0, -1.0, 0.0, 0.0, -3.0]                # the FIRST value; missing defaults to 0
    assert value(fvf(missing=7.0, factor=0.5))[:5] == [2.0, -0.5, 3.5, 0.0, -1.5]
    assert value(fvf(factor=10.0))[5] is None                            # 1e308 * 10 = inf: no value
    assert value(fvf())[5] == math.inf                                   # finite in f64, inf as f32: a value
    assert value(dict(kind="field_value_factor", field=1, factor=0.1))[1] == float(F32(10.0 * float(F32(0.1))))


@pytest.mark.parametrize("mod,want", [
    ("none", [4.0, -1.0, 0.0, 0.0, -3.0]),
    ("log", [math.log(4.0), 0.0, 0.0, 0.0, 0.0]),                        # <= 0 gives 0
    ("log1p", [math.log1p(4.0), 0.0, 0.0, 0.0, 0.0]),                    # <= -1 gives 0; log1p(0) = 0
    ("log2p", [math.log2(5.0), 0.0, 0.0, 0.0, 0.0]),
    ("sqrt", [2.0, 0.0, 0.0, 0.0, 0.0]),                                 # < 0 gives 0
    ("reciprocal", [0.25, -1.0, 0.0, 0.0, -1.0 / 3.0]),                  # == 0 gives 0
])
def test_modifier_branches(mod, want):
    got = value(dict(kind="field_value_factor", field=0, modifier=mod))[:5]
    assert got == [float(F32(w)) for w in want]


def test_modifier_just_inside_its_branch():
    m = lambda x, name: float(R.modifier(np.array([x]), name)[0])
    below, above = np.nextafter(-1.0, -2.0), np.nextafter(-1.0, 0.0)
    assert m(below, "log1p") == 0.0 and m(above, "log1p") == math.log1p(above) < -30
    assert m(-1.0, "log2p") == 0.0 and m(above, "log2p") == math.log2(above + 1.0)
    tiny = np.nextafter(0.0, 1.0)
    assert m(0.0, "log") == 0.0 and m(tiny, "log") == math.log(tiny) and m(-tiny, "log") == 0.0
    assert m(-tiny, "sqrt") == 0.0 and m(tiny, "sqrt") == math.sqrt(tiny)
    assert m(-0.0, "reciprocal") == 0.0 and m(tiny, "reciprocal") == math.inf


def test_decay_shapes():
    d = lambda **kw: dict(dict(kind="decay", field=1, origin=20.0, scale=10.0), **kw)
    # distances 20, 10, -, 10, 20, 30; offset 10 -> norm 1, 0, -, 0, 1, 2
    assert value(d(offset=10.0, function="exp", decay=0.5)) == [0.5, 1.0, None, 1.0, 0.5, 0.25]
    assert value(d(offset=10.0, function="gauss", decay=0.5)) == [0.5, 1.0, None, 1.0, 0.5, 0.0625]
    assert value(d(offset=10.0, function="linear", decay=0.5)) == [0.5, 1.0, None, 1.0, 0.5, 0.0]
    assert value(d(offset=25.0, function="exp"))[:2] == [1.0, 1.0]       # distance < offset: norm 0
    assert value(d(function="linear", decay=0.25))[5] == 0.0             # (1 - 3) * 0.75 + 0.25 < 0: clipped
    assert value(d(function="gauss", decay=1.0, scale=1e-3))[5] == 1.0   # decay 1: always 1
    assert value(d(function="gauss", decay=0.5, scale=1.0))[5] == 0.0    # 0.5 ** 900 underflows
    den = value(d(function="gauss", decay=0.5, scale=30.0 / math.sqrt(140.0)))[5]
    assert 0.0 < den < float(np.finfo(np.float32).tiny)                  # 0.5 ** 140: an f32 denormal


def combined(fsq, base):
    score, kept = R.evaluate(fsq, world(), 0, DOCS[:1], np.array([base], F32))
    return float(score[0]) if kept[0] else None


W = lambda w, **kw: dict(kind="weight", weight=w, **kw)


@pytest.mark.parametrize("mode,want", [("sum", 9.5), ("multiply", 24.0), ("max", 4.0), ("min", 1.5), ("avg", 9.5 / 3)])
def test_score_modes(mode, want):
    fsq = dict(functions=[W(4.0), W(1.5), W(4.0)], score_mode=mode, boost_mode="replace")
    assert combined(fsq, 2.0) == float(F32(F32(want)))


@pytest.mark.parametrize("mode,want", [("multiply", 6.0), ("sum", 5.0), ("replace", 3.0), ("max", 3.0), ("min", 2.0)])
def test_boost_modes(mode, want):
    assert combined(dict(functions=[W(3.0)], boost_mode=mode), 2.0) == want


def test_f32_arithmetic_step_by_step():
    a, b, c = F32(0.1), F32(0.2), F32(0.3)
    assert combined(dict(functions=[W(0.1), W(0.2), W(0.3)], score_mode="sum", boost_mode="replace"), 1.0) == float((a + b) + c)
    assert combined(dict(functions=[W(0.1), W(0.2), W(0.3)], score_mode="avg", boost_mode="replace"), 1.0) == float(((a + b) + c) / F32(3))


def test_effective_base_and_no_present_value():
    out = dict(functions=[W(3.0, filter=0)])
    assert combined(out, 0.0) == 3.0                                    # base 0 with a value: base counts as 1
    assert combined(out, 1e-8) == 3.0 and combined(out, -1e-8) == 3.0   # |base| <= epsilon too
    assert combined(out, 2e-7) == float(F32(2e-7) * F32(3.0))
    none = R.evaluate(out, world(), 0, DOCS[3:4], np.array([0.0], F32))  # the filter rejects doc 3: no value
    assert float(none[0][0]) == 0.0 and none[1][0]
    assert combined(dict(functions=[]), 0.0) == 0.0 and combined(dict(functions=[], boost=3.0), 2.0) == 6.0
    assert combined(None, 2.0) == 2.0


def test_order_of_max_boost_min_score_boost():
    fsq = dict(functions=[W(10.0)], boost_mode="replace", max_boost=4.0, min_score=4.0, boost=0.5)
    assert combined(fsq, 1.0) == 2.0                                    # capped to 4, passes min_score 4, then halved
    assert combined(dict(fsq, min_score=4.5), 1.0) is None              # min_score sees the capped value
    assert combined(dict(fsq, max_boost=None, min_score=9.0, boost=-1.0), 1.0) == -10.0  # ... and not the boosted one
    assert combined(dict(functions=[], min_score=1.0, boost=2.0), 0.5) is None
    assert combined(dict(functions=[], min_score=1.0, boost=2.0), 1.0) == 2.0


def test_a_tombstoned_doc_under_a_function_filter_has_no_value():
    cols = world()
    cols.filters[1] = [np.ones(6, bool)]
    val, has, _ = R.function_value(W(2.0, filter=1), cols, 0, DOCS)
    assert has.tolist() == [True] * 5 + [False]


def test_rounding_guard():
    f = np.float64(F32(1.5))
    up = np.float64(np.nextafter(F32(1.5), F32(2.0)))
    mid = (f + up) / 2
    assert R.safe(np.array([f, up, 0.0, 1e-300, np.inf])).all()
    assert not R.safe(np.array([mid]))[0] and not R.safe(np.array([mid * (1 + 2.0 ** -45)]))[0]
    assert R.safe(np.array([mid * (1 + 2.0 ** -39)]))[0]
    # uniformly drawn values: about 2^-16 of them are unsafe, far below the 1 % a test world may replace
    rng = np.random.default_rng(1)
    y = np.log1p(rng.uniform(0.0, 1000.0, 1 << 20))
    assert (~R.safe(y)).mean() < 1e-3


def test_total_key_orders_as_total_cmp():
    xs = np.array([-np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf], F32)
    assert (np.diff(R.total_key(xs)) > 0).all()
