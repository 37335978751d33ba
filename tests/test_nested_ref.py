"""CPU checks around nested filters: tests/nested_ref.py against the reference's own unit-test cases
(tests/golden/nested_filter_cases.json: worlds, filters and expected booleans of query/filters.rs' tests, data only);
filters.compile_nested_filter's programs against nested_ref on hand-made worlds and on the world of the GPU test; the
edges that world must have; filters.nested_columns on fast-field bytes packed here."""
import json
import os
import struct

import numpy as np
import pytest

from tests import nested_ref as R
from tests import nested_world as NW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "nested_filter_cases.json")))["cases"]
PATH_IDS = {"c": 0, "c.r": 1, "c.r.z": 2, "e": 3}
FIELD_IDS = {"cat": 0, "n": 1, "c.author": 0, "c.score": 1, "c.stars": 2, "c.r.tag": 3, "c.r.n": 4, "c.r.z.v": 5, "e.k": 6}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_ref_reproduces_the_reference_unit_tests(case):
    names = {"nested_filters_require_shared_object", "nested_filters_bind_to_parent_objects",
             "nested_numeric_filters_scope_to_same_object", "nested_and_filters_require_shared_object_in_and",
             "nested_and_filters_match_shared_object_in_and", "nested_or_filters_match_any_object",
             "nested_not_filters_negate_nested"}
    assert case["name"] in names
    for check in case["checks"]:
        if "filters" in check:   # passes_filters: a list, grouped like the children of an And
            got = R.passes_filters_at(case["world"], check["doc"], check["filters"])
        else:                    # passes_filter
            got = R.filter_matches(case["world"], check["doc"], check["filter"])
        assert got is check["expect"], (case["name"], check)


def test_the_fixture_covers_the_four_groups_of_cases():
    assert len(CASES) == 7 and sum(len(c["checks"]) for c in CASES) == 11
    assert {c["name"].split("_")[1] for c in CASES} == {"filters", "numeric", "and", "or", "not"}


def compiled_mask(flt, w, path_ids=PATH_IDS, field_ids=FIELD_IDS):
    from searchlite_amd.filters import compile_nested_filter
    fields, nested = NW.describe(path_ids, field_ids)
    prog = compile_nested_filter(flt, fields, nested)
    # children before parents, the doc level last, every other scope named exactly once by a later scope
    assert prog.scopes[-1][0] == -1 and all(p >= 0 for p, _, _ in prog.scopes[:-1])
    named = []
    for s, (_, begin, count) in enumerate(prog.scopes):
        for nd in prog.nodes[begin:begin + count]:
            if nd["kind"] == 7:
                assert nd["field"] < s
                named.append(nd["field"])
    assert sorted(named) == list(range(len(prog.scopes) - 1))
    return prog, NW.run_program(prog, w, path_ids, field_ids)


HAND = {"n_docs": 4, "kinds": dict(NW.KINDS),
        "doc": {"cat": [["news"], ["blog"], [], ["news"]], "n": [[1], [2], [3], [4]]},
        "counts": {"c": [2, 1, 0, 2], "c.r": [2, 2, 1, 0]},
        "parents": {"c.r": [[0, 1], [None, 0], [0], []]},
        "nested": {"c.author": [[["a0"], ["a2"]], [["A0", "a2"]], [], [["a2"]]],
                   "c.score": [[[9.0], [1.0]], [[1.0]], [], [[], [1.0]]],
                   "c.r.tag": [[["x"], ["y"]], [["y"], ["x"]], [["y"]], []]}}


def test_one_path_twice_in_an_and_against_the_same_in_an_or():
    a, b = NW.nest("c", NW.keq("author", "a0")), NW.nest("c", NW.f64("score", 0.0, 2.0))
    prog, got = compiled_mask(NW.AND(a, b), HAND)
    assert len(prog.scopes) == 2                                  # ONE object scope holds both children
    assert got == R.mask(HAND, NW.AND(a, b)) == [False, True, False, False]
    prog, got = compiled_mask(NW.OR(a, b), HAND)
    assert len(prog.scopes) == 3                                  # a scope each: an existential each
    assert got == R.mask(HAND, NW.OR(a, b)) == [True, True, False, True]
    # the grouping holds inside an object scope too
    inner = NW.nest("c", NW.AND(NW.nest("r", NW.keq("tag", "x")), NW.nest("r", NW.keq("tag", "y"))))
    prog, got = compiled_mask(inner, HAND)
    assert len(prog.scopes) == 3 and got == R.mask(HAND, inner) == [False, False, False, False]


def test_a_nested_under_not_and_a_doc_without_objects():
    flt = NW.NOT(NW.nest("c", NW.keq("author", "a2")))
    assert compiled_mask(flt, HAND)[1] == R.mask(HAND, flt) == [False, False, True, False]


def test_a_dotted_path_at_the_doc_level_makes_no_parent_test():
    dotted = NW.nest("c.r", NW.keq("tag", "y"))
    assert compiled_mask(dotted, HAND)[1] == R.mask(HAND, dotted) == [True, True, True, False]
    bound = NW.nest("c", NW.nest("r", NW.keq("tag", "y")))       # doc 1: the y reply has no parent; doc 2: no comment
    assert compiled_mask(bound, HAND)[1] == R.mask(HAND, bound) == [True, False, False, False]


def test_unknown_names_and_wrong_kinds_compile_to_or_of_nothing():
    for flt in (NW.nest("nope", NW.keq("author", "a0")), NW.nest("c", NW.keq("cat", "news")),
                NW.nest("c", NW.i64("score", 0, 9)), NW.nest("c", NW.f64("score", float("nan"), 1.0))):
        prog, got = compiled_mask(flt, HAND)
        assert got == R.mask(HAND, flt) == [False] * 4
        assert any(nd == dict(kind=5, arity=0) for nd in prog.nodes)
    with pytest.raises(ValueError):
        compiled_mask({"Nope": {}}, HAND)


@pytest.fixture(scope="module")
def worlds():
    return NW.build()


def test_the_gpu_world_has_the_edges_the_kernel_can_go_wrong_at(worlds):
    ws, dead = worlds
    assert [w["n_docs"] for w in ws] == [1, 33, 64, 65, 257]
    assert all(d[-1] for w, d in zip(ws, dead) if w["n_docs"] in (33, 65, 257))
    starts = {}
    for w in ws:
        c = w["counts"]["c"]
        assert {0, 1, 2, 5} <= set(c) or w["n_docs"] == 1
        if NW.BIG in c:
            starts[w["n_docs"]] = sum(c[:c.index(NW.BIG)]) % 64
    assert starts == {64: 32, 65: 31, 257: 63}                     # the 70-object doc crosses a wave from each edge
    assert set(ws[1]["counts"]["e"]) == {0} and "e" not in ws[2]["counts"]
    assert "c.r" not in ws[3]["parents"] and "c.r.n" not in ws[4]["nested"]
    short = out_of_range = unbound = fewer = False
    sizes = set()
    for w in ws:
        for d in range(w["n_docs"]):
            rows = w["parents"].get("c.r", [[]] * w["n_docs"])[d]
            short |= len(rows) < w["counts"]["c.r"][d]
            unbound |= None in rows
            out_of_range |= any(p is not None and p >= w["counts"]["c"][d] for p in rows)
            fewer |= len(w["nested"]["c.author"][d]) < w["counts"]["c"][d]
            sizes |= {len(v) for v in w["nested"]["c.author"][d]}
    assert short and out_of_range and unbound and fewer and sizes == {0, 1, 3}
    flat = lambda name: [x for w in ws for o in w["nested"].get(name, []) for v in o for x in v]
    assert {NW.I64_MIN, NW.I64_MAX, NW.TWO53 + 1, -NW.TWO53 - 1} <= set(flat("c.stars"))
    scores = flat("c.score")
    assert any(np.isnan(scores)) and NW.INF in scores and -NW.INF in scores


@pytest.mark.parametrize("family", sorted(NW.FAMILIES))
def test_every_family_passes_some_live_docs_and_fails_some(worlds, family):
    """and compile_nested_filter's program equals the reference on every doc of the world"""
    ws, dead = worlds
    passed = failed = 0
    for flt in NW.FAMILIES[family]:
        for w, gone in zip(ws, dead):
            want = np.array(R.mask(w, flt))
            assert compiled_mask(flt, w)[1] == want.tolist(), (family, flt)
            passed += int((want & ~gone).sum())
            failed += int((~want & ~gone).sum())
    assert passed > 0 and failed > 0, (family, passed, failed)


def test_every_tree_of_a_family_on_its_own_is_neither_all_true_nor_all_false(worlds):
    ws, dead = worlds
    for family, filters in NW.FAMILIES.items():
        for flt in filters:
            live = np.concatenate([np.array(R.mask(w, flt))[~gone] for w, gone in zip(ws, dead)])
            assert live.any() and not live.all(), (family, flt)


# ---- filters.nested_columns over fast-field bytes packed here (index/fastfields.rs:910-1010) ----------------
def _ffv1(columns):
    out = b"FFV1" + struct.pack("<I", len(columns))
    for name, ty, n, body in columns:
        out += struct.pack("<I", len(name)) + name.encode() + bytes([ty]) + struct.pack("<I", n) + body
    return out


def _u32(*v):
    return np.asarray(v, "<u4").tobytes()


def test_nested_columns_maps_the_five_nested_kinds_onto_the_registration_arguments():
    from searchlite_amd.filters import nested_columns
    from searchlite_amd.index_files import read_fast_fields
    dictionary = struct.pack("<I", 2) + b"".join(struct.pack("<I", len(k)) + k for k in (b"alice", b"bob"))
    buf = _ffv1([
        ("_nested_count:comment", 9, 3, _u32(2, 0, 1)),
        ("_nested_count:comment.reply", 9, 2, _u32(1, 0)),                       # shorter than the segment
        ("_nested_parent:comment.reply", 10, 2, _u32(0, 1, 1) + _u32(1)),
        ("comment.author", 8, 3, dictionary + _u32(0, 2, 2, 3) + _u32(0, 1, 1, 2) + _u32(1, 0)),
        ("comment.stars", 6, 3, _u32(0, 1, 1, 1) + _u32(0, 2) + np.asarray([2**53 + 1, -2**63], "<i8").tobytes()),
        ("comment.reply.score", 7, 1, _u32(0, 1) + _u32(0, 1) + np.asarray([0.5], "<f8").tobytes()),
        ("plain", 0, 3, bytes([1, 1, 1]) + np.asarray([1, 2, 3], "<i8").tobytes()),
    ])
    got = nested_columns(read_fast_fields(buf), 3)
    assert sorted(got["paths"]) == ["comment", "comment.reply"] and sorted(got["fields"]) == [
        "comment.author", "comment.reply.score", "comment.stars"]
    c, r = got["paths"]["comment"], got["paths"]["comment.reply"]
    assert c["parent"] is None and r["parent"] == "comment"
    assert c["counts"].tolist() == [2, 0, 1] and c["parents"] is None
    assert r["counts"].tolist() == [1, 0, 0] and r["counts"].dtype == np.uint32
    assert r["parents"][0].tolist() == [0, 1, 1, 1] and r["parents"][1].tolist() == [1]
    a, s, f = (got["fields"][n] for n in ("comment.author", "comment.stars", "comment.reply.score"))
    assert (a["path"], a["kind"], a["keys"]) == ("comment", "keyword", ["alice", "bob"])
    assert [x.tolist() for x in a["columns"]] == [[0, 2, 2, 3], [0, 1, 1, 2], [1, 0]]
    assert (s["path"], s["kind"]) == ("comment", "i64") and s["columns"][2].dtype == np.int64
    assert [x.tolist() for x in s["columns"]] == [[0, 1, 1, 1], [0, 2], [2**53 + 1, -2**63]]
    assert (f["path"], f["kind"]) == ("comment.reply", "f64")
    assert [x.tolist() for x in f["columns"]] == [[0, 1, 1, 1], [0, 1], [0.5]]   # padded to the segment's docs
