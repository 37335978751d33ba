"""tests/explain_ref.py (the reference of tests/test_gpu_explain.py must itself be right) and
searchlite_amd/explain.py, without a device:
  * the flat reference against a literal recursive transcription of evaluate_compiled_score (api/reader.rs:418-613)
    over node trees — FunctionScore{base: Expr}, ScriptScore{base: Expr} and the two nestings — on random small
    requests: values and entry order;
  * hand-derived cases: an absent function omitted, INNER against OUTER order, a base of 0.0 under the `eff` rule, a
    rescore row that is unmatched, a rescore row behind the window;
  * explain.shape() against a hand-written expected JSON."""
import types

import numpy as np
import pytest

from searchlite_amd import _native as N
from searchlite_amd import explain as E
from searchlite_amd.script import compile_script
from tests import explain_ref as X
from tests import fscore_ref, rescore_ref, script_ref

F32 = np.float32
EPS = F32(np.finfo(np.float32).eps)
N_DOCS = 12


def columns(rng):
    """one segment of 12 docs: column 3 `pop` (docs 0, 5 without a value), column 4 `age` (every doc), filter 0"""
    seg = types.SimpleNamespace(n_docs=N_DOCS, deleted=None)
    pop = [[] if d in (0, 5) else [float(rng.uniform(0.5, 50.0))] for d in range(N_DOCS)]
    age = [[int(rng.integers(0, 100))] for _ in range(N_DOCS)]
    return fscore_ref.Columns([seg], {3: ([pop], np.dtype(np.float64)), 4: ([age], np.dtype(np.int64))},
                              {0: [np.arange(N_DOCS) % 3 != 0]})


# ---- the literal transcription: a node is ("expr",), ("function_score", base node, spec) or ("script_score", base
# node, entry); evaluate() returns the score or None and appends to out_functions as the reference does ----
def combine_function_scores(values, mode):
    if not values:
        return None
    acc = values[0]
    for v in values[1:]:
        acc = {"sum": lambda a, b: F32(a + b), "avg": lambda a, b: F32(a + b), "multiply": lambda a, b: F32(a * b),
               "max": lambda a, b: F32(np.fmax(a, b)), "min": lambda a, b: F32(np.fmin(a, b))}[mode](acc, v)
    return F32(acc / F32(len(values))) if mode == "avg" else acc


def apply_boost_mode(base, fs, mode):
    return {"multiply": F32(base * fs), "sum": F32(base + fs), "replace": F32(fs), "max": F32(np.fmax(base, fs)),
            "min": F32(np.fmin(base, fs))}[mode]


def evaluate_compiled_score(node, cols, doc, leaf_score, out_functions):
    if node[0] == "expr":
        return F32(leaf_score)
    if node[0] == "function_score":
        _, base, spec = node
        base_score = evaluate_compiled_score(base, cols, doc, leaf_score, out_functions)
        if base_score is None:
            return None
        values, fn_expls = [], []
        for fn in spec.get("functions", ()):
            val, has, _ = fscore_ref.function_value(fn, cols, 0, np.array([doc]))
            if has[0]:
                values.append(F32(val[0]))
                fn_expls.append((X.function_type(fn), None if fn["kind"] == "weight" else fn["field"], F32(val[0])))
        effective_base = base_score
        if abs(effective_base) <= EPS and values:
            effective_base = F32(1.0)
        fs = combine_function_scores(values, spec.get("score_mode", "multiply"))
        combined = effective_base if fs is None else apply_boost_mode(effective_base, fs, spec.get("boost_mode", "multiply"))
        if spec.get("max_boost") is not None:
            combined = F32(np.fmin(combined, F32(spec["max_boost"])))
        if spec.get("min_score") is not None and combined < F32(spec["min_score"]):
            return None
        combined = F32(combined * F32(spec.get("boost", 1.0)))
        out_functions.extend(fn_expls)
        return combined
    assert node[0] == "script_score"
    _, base, entry = node
    base_score = evaluate_compiled_score(base, cols, doc, leaf_score, out_functions)
    if base_score is None:
        return None

    def field_value(fid):
        val, has = cols.first(fid, 0)
        return float(val[doc]) if has[doc] else None
    score = script_ref.node(entry["program"], entry.get("boost", 1.0), field_value, base_score)
    if score is None:
        return None
    out_functions.append(("script_score", None, score))
    return score


def random_function(rng):
    kind = ("weight", "field_value_factor", "decay")[int(rng.integers(0, 3))]
    fn = dict(kind=kind, filter=int(rng.integers(-1, 1)))
    if kind == "weight":
        fn["weight"] = float(rng.uniform(-2.0, 3.0))
    elif kind == "field_value_factor":
        fn.update(field=int(rng.integers(3, 5)), factor=float(rng.uniform(0.1, 2.0)),
                  modifier=("none", "sqrt", "reciprocal")[int(rng.integers(0, 3))])
        if rng.random() < 0.5:
            fn["missing"] = 2.0
        else:
            fn["missing"] = float("inf")  # a doc without a value: the product is not finite, no value
    else:
        fn.update(field=int(rng.integers(3, 5)), origin=20.0, scale=float(rng.uniform(1.0, 30.0)), offset=1.0, decay=0.5,
                  function="linear")
    return fn


def random_spec(rng):
    spec = dict(functions=[random_function(rng) for _ in range(int(rng.integers(0, 5)))],
                score_mode=("sum", "multiply", "max", "min", "avg")[int(rng.integers(0, 5))],
                boost_mode=("multiply", "sum", "replace", "max", "min")[int(rng.integers(0, 5))],
                boost=float(rng.uniform(0.5, 2.0)))
    if rng.random() < 0.3:
        spec["max_boost"] = float(rng.uniform(1.0, 40.0))
    return spec


SCRIPTS = ("_score + pop * 0.1", "_score * age - 3", "pop / (age + 1)", "-_score", "2.5")


def random_script(rng):
    return dict(program=compile_script(SCRIPTS[int(rng.integers(0, len(SCRIPTS)))], None, dict(pop=3, age=4)),
                boost=float(rng.uniform(0.5, 2.0)))


@pytest.mark.parametrize("shape", ["fscore", "script", "outer", "inner"])
def test_the_flat_chain_is_the_recursion(shape):
    rng = np.random.default_rng({"fscore": 1, "script": 2, "outer": 3, "inner": 4}[shape])
    cols = columns(rng)
    n_entries = 0
    for _ in range(40):
        spec, entry = random_spec(rng), random_script(rng)
        leaf = ("expr",)
        # SLG_SCRIPT_OUTER is script_score{query: function_score}: the function stage runs first
        tree, chain = {"fscore": (("function_score", leaf, spec), [("fscore", spec)]),
                       "script": (("script_score", leaf, entry), [("script", entry)]),
                       "outer": (("script_score", ("function_score", leaf, spec), entry), [("fscore", spec), ("script", entry)]),
                       "inner": (("function_score", ("script_score", leaf, entry), spec), [("script", entry), ("fscore", spec)])}[shape]
        base = [F32(0.0) if rng.random() < 0.2 else F32(rng.uniform(-1.0, 9.0)) for _ in range(N_DOCS)]
        got = X.explain_rows(chain, cols, [(0, d) for d in range(N_DOCS)], base)
        for d in range(N_DOCS):
            out = []
            want = evaluate_compiled_score(tree, cols, d, base[d], out)
            if want is None:
                continue  # (a dropped doc is no row of any batch)
            g = got[d]
            assert g["base"].tobytes() == base[d].tobytes()
            assert g["final"].tobytes() == want.tobytes(), (shape, d, g, want)
            assert [(t, f, v.tobytes()) for t, f, v in g["entries"]] == [(t, f, F32(v).tobytes()) for t, f, v in out]
            n_entries += len(out)
    assert n_entries > 100


W = lambda w, **kw: dict(kind="weight", weight=w, **kw)


def test_an_absent_function_is_omitted():
    cols = columns(np.random.default_rng(5))
    spec = dict(functions=[W(2.0), dict(kind="decay", field=3, origin=10.0, scale=5.0, function="linear"), W(3.0, filter=0),
                           dict(kind="field_value_factor", field=3, missing=float("inf"))], score_mode="sum", boost_mode="sum")
    # doc 0: no value of column 3 (no decay entry, the factor's product is inf: no entry), and filter 0 rejects it
    got, = X.explain_rows([("fscore", spec)], cols, [(0, 0)], [F32(1.5)])
    assert got["entries"] == [("weight", None, F32(2.0))] and got["final"] == F32(3.5) and got["base"] == F32(1.5)
    # doc 1: every function gives a value, in request order
    got, = X.explain_rows([("fscore", spec)], cols, [(0, 1)], [F32(1.5)])
    assert [(t, f) for t, f, _ in got["entries"]] == [("weight", None), ("decay_linear", 3), ("weight", None),
                                                      ("field_value_factor", 3)]


def test_inner_and_outer_order():
    cols = columns(np.random.default_rng(6))
    spec = dict(functions=[W(2.0), W(5.0)], score_mode="sum", boost_mode="multiply")
    entry = dict(program=compile_script("_score + 1"), boost=1.0)
    outer, = X.explain_rows([("fscore", spec), ("script", entry)], cols, [(0, 1)], [F32(3.0)])
    # script_score{function_score}: 3 * (2 + 5) = 21, then + 1
    assert outer["entries"] == [("weight", None, F32(2.0)), ("weight", None, F32(5.0)), ("script_score", None, F32(22.0))]
    assert outer["final"] == F32(22.0)
    inner, = X.explain_rows([("script", entry), ("fscore", spec)], cols, [(0, 1)], [F32(3.0)])
    # function_score{script_score}: 3 + 1 = 4, then * 7
    assert inner["entries"] == [("script_score", None, F32(4.0)), ("weight", None, F32(2.0)), ("weight", None, F32(5.0))]
    assert inner["final"] == F32(28.0) and inner["base"] == outer["base"] == F32(3.0)


def test_a_zero_base_keeps_its_reported_value_under_the_eff_rule():
    cols = columns(np.random.default_rng(7))
    spec = dict(functions=[W(4.0)], score_mode="sum", boost_mode="multiply")
    got, = X.explain_rows([("fscore", spec)], cols, [(0, 2)], [F32(0.0)])
    assert got["base"] == F32(0.0) and got["final"] == F32(4.0)  # eff = 1.0 enters the product only
    none = dict(functions=[W(4.0, filter=0)], score_mode="sum", boost_mode="multiply")
    got, = X.explain_rows([("fscore", none)], cols, [(0, 0)], [F32(0.0)])  # no value: no substitution
    assert got["entries"] == [] and got["final"] == F32(0.0)


def test_rescore_rows_unmatched_and_behind_the_window():
    doc, seg, score = np.array([3, 5, 2, 9], np.uint32), np.zeros(4, np.uint32), np.array([8.0, 6.0, 4.0, 2.0], F32)
    rmap = {(0, 5): F32(3.0), (0, 9): F32(50.0)}  # doc 3 and doc 2 are unmatched; doc 9 lies behind a window of 3
    rows = rescore_ref.apply_rescore(doc, seg, score, 4, rmap, 3, rescore_ref.TOTAL)
    got = X.explain_rescore(rows, 4)
    assert [int(d) for d in rows[0]] == [5, 3, 2, 9]
    assert got[0] == dict(base=F32(6.0), entries=[], final=F32(9.0), rescore=dict(rescore_score=F32(3.0), combined_score=F32(9.0)))
    assert got[1] == dict(base=F32(8.0), entries=[], final=F32(8.0), rescore=None)  # unmatched: the first-pass score
    assert got[2] == dict(base=F32(4.0), entries=[], final=F32(4.0), rescore=None)
    assert got[3] == dict(base=F32(2.0), entries=[], final=F32(2.0), rescore=None)  # behind the window, though it matches
    arrays = X.as_arrays([got], 5, with_rescore=True)
    assert arrays["rescored"].tolist() == [[1, 0, 0, 0, 0]] and arrays["combined_score"].tolist() == [[9.0, 0, 0, 0, 0]]
    assert arrays["final_score"].tolist() == [[9.0, 8.0, 4.0, 2.0, 0.0]]


def test_shape_against_a_hand_written_json():
    nf = N.MAX_EXPLAIN_FUNCS
    a = dict(base_score=np.array([[1.5, 2.0], [0.25, 0.0]], F32), final_score=np.array([[6.0, 2.0], [0.5, 0.0]], F32),
             n_functions=np.array([[3, 0], [1, 0]], np.uint32), fn_type=np.zeros((2, 2, nf), np.uint32),
             fn_field=np.full((2, 2, nf), -1, np.int32), fn_value=np.zeros((2, 2, nf), F32))
    a["fn_type"][0, 0, :3] = [N.EXPLAIN_WEIGHT, N.EXPLAIN_DECAY_GAUSS, N.EXPLAIN_SCRIPT_SCORE]
    a["fn_field"][0, 0, 1] = 7
    a["fn_value"][0, 0, :3] = [2.0, 0.5, 6.0]
    a["fn_type"][1, 0, 0], a["fn_field"][1, 0, 0], a["fn_value"][1, 0, 0] = N.EXPLAIN_FIELD_VALUE_FACTOR, 4, 2.0
    want = [[{"base_score": 1.5, "functions": [{"type": "weight", "value": 2.0},
                                               {"type": "decay_gauss", "value": 0.5, "field": "published"},
                                               {"type": "script_score", "value": 6.0}], "final_score": 6.0},
             {"base_score": 2.0, "functions": [], "final_score": 2.0}],
            [{"base_score": 0.25, "functions": [{"type": "field_value_factor", "value": 2.0, "field": "popularity"}],
              "final_score": 0.5}]]
    names = {7: "published", 4: "popularity"}
    assert E.shape(a, names, counts=[2, 1]) == want
    assert E.shape(a, names.get, counts=[2, 1]) == want
    assert len(E.shape(a, names)[1]) == 2  # without counts every row of the arrays is shaped
    # a rescore batch: the part is present only for a rescored row
    a.update(rescored=np.array([[1, 0], [0, 0]], np.uint32), rescore_score=np.array([[4.5, 0], [0, 0]], F32),
             combined_score=np.array([[6.0, 0], [0, 0]], F32))
    got = E.shape(a, names, counts=[2, 1])
    assert got[0][0]["rescore"] == {"rescore_score": 4.5, "combined_score": 6.0, "functions": []}
    assert "rescore" not in got[0][1] and "rescore" not in got[1][0]
    assert sorted(E.TYPE_NAMES.values()) == sorted(X.TYPES) and [E.TYPE_NAMES[i] for i in range(6)] == list(X.TYPES)
