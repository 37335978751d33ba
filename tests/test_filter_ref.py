"""tests/filter_ref.py against hand-derived cases taken from the reference's own tests (query/filters.rs:
keyword_filters_are_case_insensitive, evaluates_all_filter_types), the empty And / Or, Not over a doc without a
value; and searchlite_amd.filters.compile_filter's programs (ordinal resolution, postfix order, Nested) against the
same evaluation."""
import numpy as np
import pytest

from tests import filter_ref as FR

from searchlite_amd import _native as N
from searchlite_amd.filters import compile_filter

EQ = lambda field, value: {"KeywordEq": {"field": field, "value": value}}
IN = lambda field, values: {"KeywordIn": {"field": field, "values": values}}
I64 = lambda field, lo, hi: {"I64Range": {"field": field, "min": lo, "max": hi}}
F64 = lambda field, lo, hi: {"F64Range": {"field": field, "min": lo, "max": hi}}


def one_doc_fields(**cols):
    """name=(kind, keys or None, the doc's values): one segment of one doc"""
    return {name: dict(kind=kind, keys=keys, id=i, docs=[[list(vals)]])
            for i, (name, (kind, keys, vals)) in enumerate(cols.items())}


def passes(flt, fields, nested=None):
    return bool(FR.eval_filter(flt, fields, 0, 1, nested)[0])


def program_passes(flt, fields, nested_ids=None, filter_pass=None):
    prog = compile_filter(flt, fields, nested=None if nested_ids is None else (lambda path, f: nested_ids[path]))
    by_id = {f["id"]: f for f in fields.values()}
    return bool(FR.eval_program(prog.nodes, prog.ords, by_id, filter_pass or {}, 0, 1)[0])


# filters.rs keyword_filters_are_case_insensitive: cat = "News", topic = "ÜMLAUT", tags = ["Ümlaut", "NEWS"]
CASE_FIELDS = one_doc_fields(cat=("keyword", ["News"], [0]), topic=("keyword", ["ÜMLAUT"], [0]),
                             tags=("keyword", ["Ümlaut", "NEWS"], [0, 1]))
CASE_FILTERS = [EQ("cat", "news"), EQ("topic", "ümlaut"), IN("tags", ["ümlaut", "news"]), IN("cat", ["sports", "NEWS"])]


@pytest.mark.parametrize("check", [passes, program_passes])
def test_keyword_filters_are_case_insensitive(check):
    for f in CASE_FILTERS:
        assert check(f, CASE_FIELDS), f
    assert check({"And": CASE_FILTERS}, CASE_FIELDS)
    assert not check(EQ("cat", "other"), CASE_FIELDS)  # the reference's `rejecting`
    assert not check({"And": CASE_FILTERS + [EQ("cat", "other")]}, CASE_FIELDS)


# filters.rs evaluates_all_filter_types: cat = "news", year = 2024, score = 0.75
ALL_FIELDS = one_doc_fields(cat=("keyword", ["news"], [0]), year=("i64", None, [2024]), score=("f64", None, [0.75]))
ALL_FILTERS = [EQ("cat", "news"), IN("cat", ["sports", "news"]), I64("year", 2020, 2025), F64("score", 0.5, 1.0)]


@pytest.mark.parametrize("check", [passes, program_passes])
def test_evaluates_all_filter_types(check):
    for f in ALL_FILTERS:
        assert check(f, ALL_FIELDS), f
    assert check({"And": ALL_FILTERS}, ALL_FIELDS)
    assert not check(I64("year", 2025, 2030), ALL_FIELDS)  # the reference's `rejecting`: 2024 is below 2025
    assert check(I64("year", 2024, 2024), ALL_FIELDS) and not check(I64("year", 2025, 2024), ALL_FIELDS)
    assert not check(F64("score", 0.76, 1.0), ALL_FIELDS) and check(F64("score", 0.75, 0.75), ALL_FIELDS)


@pytest.mark.parametrize("check", [passes, program_passes])
def test_a_field_of_another_kind_or_none_matches_nothing(check):
    """fastfields.rs matches_*: `_ => false`"""
    assert not check(EQ("year", "2024"), ALL_FIELDS)
    assert not check(I64("score", 0, 1), ALL_FIELDS) and not check(F64("year", 0.0, 1e9), ALL_FIELDS)
    assert not check(EQ("nope", "x"), ALL_FIELDS) and check({"Not": EQ("nope", "x")}, ALL_FIELDS)
    assert not check(F64("score", float("nan"), 1.0), ALL_FIELDS)  # every comparison with NaN is false


@pytest.mark.parametrize("check", [passes, program_passes])
def test_empty_and_passes_and_empty_or_does_not(check):
    assert check({"And": []}, ALL_FIELDS)       # passes_filters_at over no filter
    assert not check({"Or": []}, ALL_FIELDS)    # any() over no child
    assert not check({"Not": {"And": []}}, ALL_FIELDS) and check({"Not": {"Or": []}}, ALL_FIELDS)


@pytest.mark.parametrize("check", [passes, program_passes])
def test_not_over_a_doc_without_a_value(check):
    fields = one_doc_fields(cat=("keyword", ["news"], []), year=("i64", None, []), score=("f64", None, []))
    for leaf in (EQ("cat", "news"), IN("cat", ["news"]), I64("year", -2**63, 2**63 - 1),
                 F64("score", float("-inf"), float("inf"))):
        assert not check(leaf, fields), leaf
        assert check({"Not": leaf}, fields), leaf
    gone = {name: dict(f, docs=[None]) for name, f in fields.items()}  # the segment has no value at all
    assert not passes(EQ("cat", "news"), gone) and passes({"Not": EQ("cat", "news")}, gone)


def test_multi_valued_docs_pass_on_any_value():
    fields = {"n": dict(kind="f64", keys=None, id=0, docs=[[[1.0, 9.0], [], [float("nan")], [5.0]]])}
    got = FR.eval_filter(F64("n", 4.0, 9.0), fields, 0, 4)
    assert got.tolist() == [True, False, False, True]
    prog = compile_filter({"Not": F64("n", 4.0, 9.0)}, fields)
    assert FR.eval_program(prog.nodes, prog.ords, {0: fields["n"]}, {}, 0, 4).tolist() == [False, True, True, False]


def test_ordinal_resolution():
    """Several dictionary keys may fold to one value: every one of them is in the node's set, in dictionary order;
    repeated request values add nothing; a value no key equals leaves an empty set, which passes nothing."""
    keys = ["news", "Sports", "NEWS", "ümlaut", "ÜMLAUT", "straße", "STRASSE", "\u212aelvin"]
    fields = {"cat": dict(kind="keyword", keys=keys, id=7, docs=[[[0]]])}
    prog = compile_filter(EQ("cat", "News"), fields)
    assert prog.ords == [0, 2]
    assert prog.nodes == [dict(kind=N.FILTER_KEYWORD_IN, field=7, ord_begin=0, n_ords_in=2)]
    assert compile_filter(EQ("cat", "Ümlaut"), fields).ords == [3, 4]
    # to_lowercase is not a case FOLD: "straße" and "STRASSE" stay apart, as in the reference
    assert compile_filter(EQ("cat", "STRASSE"), fields).ords == [6]
    assert compile_filter(EQ("cat", "strasse"), fields).ords == [6]
    # one side not ASCII: to_lowercase on both (KELVIN SIGN lowers to "k")
    assert compile_filter(EQ("cat", "Kelvin"), fields).ords == [7]
    prog = compile_filter({"Or": [IN("cat", ["sports", "news", "SPORTS"]), EQ("cat", "absent")]}, fields)
    assert prog.ords == [0, 1, 2]
    assert prog.nodes == [dict(kind=N.FILTER_KEYWORD_IN, field=7, ord_begin=0, n_ords_in=3),
                          dict(kind=N.FILTER_KEYWORD_IN, field=7, ord_begin=3, n_ords_in=0),
                          dict(kind=N.FILTER_OR, arity=2)]


def test_ranges_and_postfix_order():
    fields = {"year": dict(kind="i64", id=3), "score": dict(kind="f64", id=4)}
    prog = compile_filter({"And": [I64("year", -2**63, 2**63 - 1), {"Not": F64("score", float("-inf"), 0.5)}]}, fields)
    assert prog.nodes == [dict(kind=N.FILTER_RANGE_I64, field=3, lo_i=-2**63, hi_i=2**63 - 1),
                          dict(kind=N.FILTER_RANGE_F64, field=4, lo_f=float("-inf"), hi_f=0.5),
                          dict(kind=N.FILTER_NOT), dict(kind=N.FILTER_AND, arity=2)]
    assert prog.ords == []


def test_nested_goes_through_the_callback_or_is_unsupported():
    fields = {"cat": dict(kind="keyword", keys=["news"], id=0, docs=[[[0]]])}
    a, b = EQ("author", "alice"), EQ("tag", "rust")
    flt = {"And": [EQ("cat", "news"), {"Nested": {"path": "comment", "filter": a}},
                   {"Nested": {"path": "comment", "filter": b}}, {"Nested": {"path": "review", "filter": a}}]}
    with pytest.raises(N.SlgError) as ei:
        compile_filter(flt, fields)
    assert ei.value.code == N.ERR_UNSUPPORTED
    calls = []

    def nested(path, f):
        calls.append((path, f))
        return 40 + len(calls)

    prog = compile_filter(flt, fields, nested=nested)
    # filters.rs nested_filters_require_shared_object: the Nested children of one path hold for ONE object
    assert calls == [("comment", {"And": [a, b]}), ("review", a)]
    assert prog.nodes == [dict(kind=N.FILTER_KEYWORD_IN, field=0, ord_begin=0, n_ords_in=1),
                          dict(kind=N.FILTER_ID, filter_id=41), dict(kind=N.FILTER_ID, filter_id=42),
                          dict(kind=N.FILTER_AND, arity=3)]
    masks = {41: [np.array([True])], 42: [np.array([False])]}
    assert not FR.eval_program(prog.nodes, prog.ords, {0: fields["cat"]}, masks, 0, 1)[0]
    seen = []
    ref = FR.eval_filter(flt, fields, 0, 1, nested=lambda path, f, seg: (seen.append((path, f)), np.array([True]))[1])
    assert ref[0] and seen == calls
    prog = compile_filter({"Not": {"Nested": {"path": "comment", "filter": a}}}, fields, nested=lambda p, f: 5)
    assert prog.nodes == [dict(kind=N.FILTER_ID, filter_id=5), dict(kind=N.FILTER_NOT)]


def test_malformed_filters():
    for bad in ({}, {"And": [], "Or": []}, {"Xor": []}, [1], "x"):
        with pytest.raises(ValueError):
            compile_filter(bad, {})
