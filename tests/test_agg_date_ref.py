"""tests/agg_date_ref.py against the results the reference's own tests record (tests/golden/agg_date_cases.json),
and searchlite_amd.aggs (agg_spec's parsing, shape) against the helper on hand-made tables.  No device."""
import copy
import json
import os

import numpy as np
import pytest

from tests import agg_date_ref as D

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agg_date_cases.json")
with open(GOLD) as fh:
    CASES = {c["name"]: c for c in json.load(fh)["cases"]}


def prepared(case):
    """the case's request with its filter aggregations named for the helper -> (request, passes)"""
    req = copy.deepcopy(case["request"])
    for name, body in req.items():
        if body["type"] == "filter":
            body["filter"] = {"name": name}
    return req, case.get("filter_passes", {})


def all_docs(columns):
    per_seg = next(iter(columns.values()))
    return [(s, d) for s in range(len(per_seg)) for d in range(len(per_seg[s]))]


def check_expected(got, want, what):
    assert got["type"] == want["type"], what
    if "keys" in want:
        assert [b["key"] for b in got["buckets"]] == want["keys"], what
        assert all(type(b["key"]) is type(k) for b, k in zip(got["buckets"], want["keys"])), what
    if "doc_counts" in want:
        assert [b["doc_count"] for b in got["buckets"]] == want["doc_counts"], what
    for f in ("keyed", "value", "doc_count"):
        if f in want:
            assert got[f] == want[f], (what, f)
    for name, sub in want.get("aggregations", {}).items():
        check_expected(got["aggregations"][name], sub, f"{what}.{name}")


def test_helper_calendar_and_ceil_semantics():
    from searchlite_amd import aggs as A, _native as N
    fixed = D.config({"fixed_interval": "1s", "offset": "0.5s"})
    assert [D.bucket_start(v, fixed) for v in (0, 500, 501, 1000, 1600, -500, -501)] == \
        [500, 500, 1500, 1500, 2500, -500, -500]  # ceil: a boundary is its own bucket, else the NEXT boundary
    week = D.config({"calendar_interval": "week"})
    assert D.bucket_start(-1, week) == -3 * 86_400_000  # 1969-12-31 lies in the week of Monday 1969-12-29
    assert D.dense_id(-1, week) == 0 and D.dense_id(-3 * 86_400_000 - 1, week) == -1
    assert D.dense_id(4 * 86_400_000 - 1, week) == 0 and D.dense_id(4 * 86_400_000, week) == 1  # 01-04 | 01-05
    month = D.config({"calendar_interval": "1M"})  # "1m" as a calendar interval is a month
    assert month["unit"] == "month" and D.dense_id(-1, month) == -1 and D.bucket_start(-1, month) == -31 * 86_400_000
    assert D.config({"calendar_interval": "day", "fixed_interval": "1h"})["unit"] == "day"  # calendar wins
    assert D.as_i64(-0.5) == 0 and D.as_i64(-1.5) == -1
    # the library's integer restatement (aggs.bucket_start, add_interval, bucket_key) against the helper's datetime
    rng = np.random.default_rng(3)
    instants = [int(v) for v in rng.integers(-62_135_596_800_000 + 3_600_000, 253_402_300_799_999, 400)] + \
        [0, -1, 1, -3 * 86_400_000, 4 * 86_400_000, 951_782_400_000, 1_709_164_800_000]
    for unit, code in (("day", N.DATE_DAY), ("week", N.DATE_WEEK), ("month", N.DATE_MONTH),
                       ("quarter", N.DATE_QUARTER), ("year", N.DATE_YEAR)):
        for off in (0, 3_600_000):
            cfg = dict(unit=unit, step=0, offset=off)
            for v in instants:
                key = D.bucket_start(v, cfg)
                assert A.bucket_start(v, off, code, 0) == key, (unit, off, v)
                assert A.bucket_key(D.dense_id(v, cfg), off, code, 0) == key, (unit, off, v)
                assert A.add_interval(key, code, 0) == D.add_interval(key, cfg), (unit, off, v)
    for step, off in ((1, 0), (7, -3), (1000, 500), (86_400_000, 0)):
        cfg = dict(unit=None, step=step, offset=off)
        for v in instants[:50] + [off + 5 * step, off + 5 * step + 1, off - 5 * step - 1]:
            assert A.bucket_start(v, off, N.DATE_FIXED, step) == D.bucket_start(v, cfg)
            assert A.bucket_key(D.dense_id(v, cfg), off, N.DATE_FIXED, step) == D.bucket_start(v, cfg)


# ---- searchlite_amd.aggs against the helper ---------------------------------------------------------------------
KEYS = {"tag": ["hobby", "tech", "work"]}
DAY = 86_400_000


def lib_fields(columns, filter_ids=None):
    from searchlite_amd import aggs as A
    fields = {f: {"id": i, "keys": KEYS.get(f)} for i, f in enumerate(sorted(columns))}
    if filter_ids is not None:
        fields[A.FILTERS] = lambda body: filter_ids[body["name"]]
    return fields


def shape_matches_helper(req, columns, passes=None, docs=None):
    """aggs.shape over the helper's own dense tables == the helper's response"""
    from searchlite_amd import aggs as A
    passes = passes or {}
    plan = A.agg_spec(req, lib_fields(columns, {n: i for i, n in enumerate(sorted(passes))}))
    docs = all_docs(columns) if docs is None else docs
    states = D.run(req, columns, passes, docs)
    layout = D.ref_layout(plan.nodes, columns, KEYS)
    tables = [t[None] for t in D.dense(plan.nodes, layout, states, KEYS)]
    got, want = A.shape(plan, layout, tables, 0), D.respond(req, states)
    assert got == want
    return plan, got


@pytest.mark.parametrize("name", list(CASES))
def test_helper_and_shape_give_the_reference_s_recorded_results(name):
    case = CASES[name]
    req, passes = prepared(case)
    resp = D.respond(req, D.run(req, case["columns"], passes, all_docs(case["columns"])))
    _, got = shape_matches_helper(req, case["columns"], passes)
    for agg, want in case["expected"].items():
        check_expected(resp[agg], want, f"helper {name}.{agg}")
        check_expected(got[agg], want, f"shape {name}.{agg}")


COLS = {"ts": [[[0], [DAY - 1, DAY], [], [40 * DAY + 5], [-1], [3 * DAY, 3 * DAY + 7]], [[100 * DAY], [], [-40 * DAY]]],
        "x": [[[0.5], [-0.5, 2.25], [], [1.0], [3.0], []], [[-1.5], [4.0], [0.25]]],
        "tag": [[["tech"], ["tech", "work"], [], ["hobby"], ["tech"], ["work"]], [["hobby"], [], ["tech"]]]}
PASSES = {"odd": [[False, True, False, True, False, True], [False, True, False]],
          "all": [[True] * 6, [True] * 3]}

SHAPES = {
    "extended_bounds_with_offset": {"h": {"type": "date_histogram", "field": "ts", "calendar_interval": "month",
                                          "offset": "1h", "extended_bounds": {"min": "1969-11-15T00:00:00Z",
                                                                              "max": "1970-06-01T00:00:00Z"}}},
    "fixed_day_offset_bounds": {"h": {"type": "date_histogram", "field": "ts", "fixed_interval": "1d", "offset": "6h",
                                      "missing": "1970-01-03T00:00:00Z",
                                      "extended_bounds": {"min": "-172800000", "max": "1970-01-06T00:00:00Z"}}},
    "hard_bounds_min_doc_count": {"h": {"type": "date_histogram", "field": "ts", "calendar_interval": "week",
                                        "min_doc_count": 1, "hard_bounds": {"min": "0", "max": "1970-02-15T00:00:00Z"}}},
    "quarter_year": {"q": {"type": "date_histogram", "field": "ts", "calendar_interval": "quarter", "missing": 86400000.0},
                     "y": {"type": "date_histogram", "field": "ts", "calendar_interval": "1y",
                           "extended_bounds": {"min": "1968-02-29T00:00:00Z", "max": "1972-01-01T00:00:00Z"}}},
    "date_children": {"h": {"type": "date_histogram", "field": "ts", "calendar_interval": "month",
                            "aggs": {"s": {"type": "stats", "field": "x"}, "t": {"type": "terms", "field": "tag"},
                                     "c": {"type": "cardinality", "field": "tag"},
                                     "f": {"type": "filter", "filter": {"name": "odd"}},
                                     "r": {"type": "percentile_ranks", "field": "x", "values": [0.0, 2.0]},
                                     "v": {"type": "value_count", "field": "x", "missing": 7}}}},
    "parents_of_dates": {"t": {"type": "terms", "field": "tag", "missing": "none",
                               "aggs": {"h": {"type": "date_histogram", "field": "ts", "fixed_interval": "30d"}}},
                         "f": {"type": "filter", "filter": {"name": "odd"},
                               "aggs": {"h": {"type": "date_histogram", "field": "ts", "calendar_interval": "year"},
                                        "s": {"type": "stats", "field": "x", "missing": 1.5}}},
                         "g": {"type": "filter", "filter": {"name": "all"}}},
    "date_range_and_value_count": {"r": {"type": "date_range", "field": "ts", "missing": 5,
                                         "ranges": [{"to": "1970-01-02T00:00:00Z"},
                                                    {"key": "later", "from": "1970-01-02T00:00:00Z"},
                                                    {"from": "86399999", "to": "not a date"}],
                                         "aggs": {"n": {"type": "value_count", "field": "x"}}},
                                   "n": {"type": "value_count", "field": "ts", "missing": "12"}},
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_equals_the_helper(name):
    plan, got = shape_matches_helper(SHAPES[name], COLS, PASSES)
    if name == "extended_bounds_with_offset":
        keys = [b["key"] for b in got["h"]["buckets"]]
        # the walk starts at bucket_start(min) = 1969-11-01 + 1 h; add_calendar re-truncates to midnight, so the zero
        # buckets behind it lose the offset, while buckets that docs were counted in keep it
        hour = 3_600_000
        assert keys[0] == -61 * DAY + hour and -31 * DAY in keys and -31 * DAY + hour in keys
        assert 31 * DAY in keys and 31 * DAY + hour in keys and keys == sorted(keys)
        assert all(isinstance(k, int) for k in keys)


def test_agg_spec_parsing_and_request_checks():
    from searchlite_amd import aggs as A, _native as N
    fields = lib_fields(COLS, {"odd": 4})
    dh = lambda **kw: {"h": dict({"type": "date_histogram", "field": "ts"}, **kw)}
    for spec, secs in (("1s", 1.0), ("1.5s", 1.5), ("250ms", 0.25), ("2m", 120.0), ("1h", 3600.0), ("1d", 86400.0),
                       ("2w", 1209600.0), ("30", 30.0), (".5s", 0.5), ("1.", 1.0)):
        assert A.parse_interval_seconds(spec) == secs == D.parse_interval_seconds(spec), spec
    for spec in ("", "s", "-1s", "1x", "1 s", "1.2.3s", "1M", "."):
        assert A.parse_interval_seconds(spec) is None and D.parse_interval_seconds(spec) is None, spec
    for text in ("1970-01-01T00:00:03Z", "2024-02-29T12:00:00.5+02:00", "1969-12-31T23:59:59.999Z", "500", "-1.5e3",
                 "0001-01-01T00:00:00Z", "9999-12-31T23:59:59.999Z", "2023-02-29T00:00:00Z", "yesterday", "1 000"):
        assert A.parse_date(text) == D.parse_date(text), text
    assert A.parse_date("1969-12-31T23:59:59.999Z") == -1.0 and A.parse_date("2023-02-29T00:00:00Z") is None
    n = A.agg_spec(dh(fixed_interval="1.0015s", offset="0.5s", missing="1970-01-01T00:00:01Z",
                      hard_bounds={"min": "-5", "max": "1970-01-02T00:00:00Z"}), fields).spec.nodes[0]
    assert (n.kind, n.calendar_unit, n.date_step, n.date_offset) == (N.AGG_DATE_HISTOGRAM, N.DATE_FIXED, 1001, 500)
    assert (n.has_missing, n.missing, n.has_hard_bounds, n.date_hard_min, n.date_hard_max) == (1, 1000.0, 1, -5, DAY)
    n = A.agg_spec(dh(calendar_interval="1M", fixed_interval="1h"), fields).spec.nodes[0]  # calendar wins; 1m: month
    assert (n.calendar_unit, n.has_missing, n.has_hard_bounds) == (N.DATE_MONTH, 0, 0)
    for unit, code in (("day", 1), ("1w", 2), ("Month", 3), ("QUARTER", 4), ("1y", 5)):
        assert A.agg_spec(dh(calendar_interval=unit), fields).spec.nodes[0].calendar_unit == code
    for bad, word in ((dh(), "requires"), (dh(calendar_interval="fortnight"), "not supported"),
                      (dh(calendar_interval="2d"), "not supported"), (dh(fixed_interval="soon"), "invalid"),
                      (dh(calendar_interval="day", fixed_interval="1x"), "invalid"),
                      (dh(fixed_interval="1s", offset="-3"), "offset"),
                      (dh(fixed_interval="1s", extended_bounds={"min": "then", "max": "5"}), "extended_bounds.min"),
                      (dh(fixed_interval="1s", hard_bounds={"min": "1", "max": "now"}), "hard_bounds.max"),
                      (dh(fixed_interval="1s", hard_bounds={"min": "6", "max": "5"}), "min > max"),
                      (dh(fixed_interval="1s", extended_bounds={"min": "1970-01-01T00:00:01Z", "max": "999"}), "min > max")):
        with pytest.raises(ValueError, match=word):
            A.agg_spec(bad, fields)
    # filter: by a registered id through fields[FILTERS]; without the mapping it is not built
    flt = {"f": {"type": "filter", "filter": {"name": "odd"}, "aggs": {"s": {"type": "stats", "field": "x"}}}}
    plan = A.agg_spec(flt, fields)
    assert (plan.spec.nodes[0].kind, plan.spec.nodes[0].filter, plan.spec.nodes[1].parent) == (N.AGG_FILTER, 4, 0)
    with pytest.raises(ValueError, match="filter"):
        A.agg_spec(flt, {k: v for k, v in fields.items() if k != A.FILTERS})
    # the host mappings
    dr = A.agg_spec(SHAPES["date_range_and_value_count"], fields)
    n = dr.spec.nodes[1]
    assert [x["type"] for x in dr.nodes] == ["value_count", "date_range", "value_count"]
    assert (n.kind, n.n_ranges, n.has_missing, n.missing) == (N.AGG_RANGE, 3, 1, 5.0)
    assert list(n.from_[:3]) == [float("-inf"), float(DAY), 86399999.0] and list(n.to[:3]) == [float(DAY), float("inf"), float("inf")]
    assert (dr.spec.nodes[0].kind, dr.spec.nodes[0].missing, dr.spec.nodes[2].parent) == (N.AGG_STATS, 12.0, 1)
    with pytest.raises(ValueError, match="two levels"):  # a third level stays on the CPU
        A.agg_spec({"f": {"type": "filter", "filter": {"name": "odd"}, "aggs": {
            "h": dict(dh(calendar_interval="day")["h"], aggs={"s": {"type": "stats", "field": "x"}})}}}, fields)
