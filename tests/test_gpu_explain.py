"""explain on the device (slg_batch_explain; PreparedBatch.explain) through the C ABI against tests/explain_ref.py.
Tolerance 0 on bits: base scores, final scores, entry counts, types, field ids and values are identical to the
reference, and rows at or beyond a query's count are zero.

What the reference is independent of: the base score of a row comes from the oracle's exhaustive run
(fscore_ref.all_candidates), never from the device; the entries and the final score from explain_ref over the chain
of stages.  The rows that are explained are the batch's own (what other files check), and for every explained row of
a batch without rescore the final score must be the row's fetched score, bit for bit — the feature's own cross-check.

Transcendental results round the same everywhere because the columns are drawn through fscore_ref.unsafe_draws
(tests/test_gpu_fscore.py: safe_column), asserted again before the device is touched."""
import numpy as np
import pytest

from searchlite_amd import _native as N
from searchlite_amd import explain as E
from tests import bool_ref, explain_ref as X, fscore_ref, rescore_ref
from tests.script_worlds import World
from tests.test_gpu_bool import MUST, MUST_NOT, SHOULD, csr, dead_bitmap, same
from tests.test_gpu_fscore import AGE, DECAY, FVF, POP, W, on, safe_column
from tests.util import _append_lists, random_queries, random_segment

pytestmark = pytest.mark.gpu
F32 = np.float32
NO_TERM = 0xFFFFFFFF
KS = (11, 257, 1025)
ROWS = (1, 255, 256, 257, 1024)  # and a value above a query's count: every k here is one for some query


@pytest.fixture(scope="module")
def A(oracle):
    """two segments of 300 and 200 docs, vocab 40, tombstones in both.  Columns: `pop` f64, 0-3 values per doc (some
    docs have none), `age` i64 one value per doc, `half` f64 whose second segment has no value at all; filter f0"""
    import searchlite_amd as sa
    rng = np.random.default_rng(29)
    segs = [random_segment(rng, 300, 40, 6), random_segment(rng, 200, 40, 6)]
    segs[0].deleted = dead_bitmap(rng, 300, 0.1)
    segs[1].deleted = dead_bitmap(rng, 200, 0.15)
    Wd = World(sa, oracle, segs)
    Wd.add_field("pop", safe_column(lambda: [float(rng.uniform(0.1, 1000.0)) for _ in range(int(rng.integers(0, 4)))],
                                    segs, POP, np.float64), np.float64)
    Wd.add_field("age", safe_column(lambda: [int(rng.integers(0, 5001))], segs, AGE, np.int64), np.int64)
    Wd.add_field("half", [[[float(rng.uniform(1.0, 9.0))] if rng.random() < 0.7 else [] for _ in range(300)], None], np.float64)
    Wd.add_filter("f0", [rng.random(s.n_docs) < 0.5 for s in segs])
    Wd.qs16 = random_queries(rng, 16, 3, 40, n_segs=2, weights=True)
    Wd.qs12 = random_queries(rng, 6, 12, 40, n_segs=2, weights=True)
    Wd.rng = rng
    yield Wd
    Wd.ix.close()


@pytest.fixture(scope="module")
def Bw(oracle):
    """one segment of 6000 docs with appended lists of df 1, 64, 65, 4096 and 6000; the first and last postings of
    the lists of 64, 65 and 4096 are docs 0 and 5999, which `top` puts on top of every query with doc 4321 (the df-1
    list): the edges of the search are explained rows.  Column `rank` i64: the doc id"""
    import searchlite_amd as sa
    rng = np.random.default_rng(31)
    n, vocab = 6000, 40
    base = random_segment(rng, n, vocab, 6)
    ends = np.array([0, n - 1], np.uint32)

    def with_ends(df):
        inner = rng.choice(np.arange(1, n - 1), size=df - 2, replace=False)
        return np.sort(np.concatenate([ends, inner.astype(np.uint32)])).astype(np.uint32)

    lists = {"all": np.arange(n, dtype=np.uint32), "top": np.array([0, 4321, n - 1], np.uint32),
             "one": np.array([4321], np.uint32), "d64": with_ends(64), "d65": with_ends(65), "d4096": with_ends(4096)}
    seg = _append_lists(base, [(d, rng.integers(1, 4, size=len(d))) for d in lists.values()])
    Wd = World(sa, oracle, [seg])
    Wd.T = {name: vocab + i for i, name in enumerate(lists)}
    Wd.add_field("rank", [[[int(d)] for d in range(n)]], np.int64)
    Wd.lists = lists
    yield Wd
    Wd.ix.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_CANDS = {}


def candidates(Wd, qs, plans):
    """one exhaustive oracle run per (query set, score plans), shared by the checks (World.cands tells plans apart by
    their argument names alone)"""
    key = (id(Wd), id(qs), tuple((n, np.asarray(v).tobytes()) for n, v in sorted((plans or {}).items())))
    if key not in _CANDS:
        _CANDS[key] = (qs, fscore_ref.all_candidates(Wd.oracle, Wd.segs, *qs, **(plans or {})))
    return _CANDS[key][1]


def check(Wd, b, qs, chains, rows, what, plans=None):
    """the batch b (run) explained at `rows` against the reference over its own rows -> (fetched, explained)"""
    got = b.fetch()
    ex = b.explain(rows)
    nq, k = len(got[3]), got[0].shape[1]
    n = [min(rows, int(got[3][q]), k) for q in range(nq)]
    row_list = [[(int(got[1][q, i]), int(got[0][q, i])) for i in range(n[q])] for q in range(nq)]
    want = X.as_arrays(X.explain(candidates(Wd, qs, plans), chains, Wd.cols, row_list), rows)
    assert sorted(ex) == sorted(want)
    for name in want:
        assert ex[name].shape == want[name].shape, name
        if not np.array_equal(bits(ex[name]), bits(want[name])):
            q, r = [int(x[0]) for x in np.nonzero(bits(ex[name]) != bits(want[name]))[:2]]
            raise AssertionError(f"{what}: {name} differs at query {q} row {r}: {ex[name][q, r]} != {want[name][q, r]} "
                                 f"(n_functions {ex['n_functions'][q, r]} / {want['n_functions'][q, r]})")
    for q in range(nq):  # the feature's own cross-check: the end of the chain is the row's score
        assert np.array_equal(bits(ex["final_score"][q, :n[q]]), bits(got[2][q, :n[q]])), f"{what}: final != row score, query {q}"
        assert not ex["base_score"][q, n[q]:].any() and not ex["n_functions"][q, n[q]:].any()
    return got, ex


def explain_all_rows(Wd, b, qs, chains, what, plans=None, rows=ROWS):
    b.run()
    out = None
    for r in rows:
        out = check(Wd, b, qs, chains, r, f"{what} rows={r}", plans)
    return out


# ---------------------------------------------------------------------------------------------- base scores
@pytest.mark.parametrize("k", KS)
def test_plain_flat_sum_on_both_scoring_kernels(A, k):
    """three terms (the few-term kernel) and twelve (the many-term kernel): no stage, so base == final == row score"""
    for qs, name in ((A.qs16, "3 terms"), (A.qs12, "12 terms")):
        nq = len(qs[0]) - 1
        with A.ix.prepare(*qs, k) as b:
            got, ex = explain_all_rows(A, b, qs, [[]] * nq, f"{name} k={k}")
            assert not ex["n_functions"].any() and np.array_equal(bits(ex["base_score"]), bits(ex["final_score"]))
            n = min(k, 1024)
            assert np.array_equal(bits(ex["base_score"][:, :n]), bits(got[2][:, :n]))
            if k == 11:
                assert (got[3] == k).all()  # rows 255 .. 1024 lie above every query's count
            if k == 1025:
                assert (got[3] < 1024).all() and (name == "3 terms" or got[3].max() > 256)  # counts between the row values


def test_sum_of_two_term_leaves_and_dismax_with_an_absent_leaf(A):
    nq = 16
    two = dict(q_leaf=np.tile([0, 0, 1], nq), q_plan=np.zeros(nq, np.int32), q_tie=np.zeros(nq, F32))
    with A.ix.prepare(*A.qs16, 257, **two) as b:
        explain_all_rows(A, b, A.qs16, [[]] * nq, "Sum, two terms in a leaf", two, rows=(257,))
    dis = dict(q_leaf=np.tile([0, 0, 1], nq), q_plan=np.full(nq, 1, np.int32), q_tie=np.full(nq, 0.3, F32))
    with A.ix.prepare(*A.qs16, 257, **dis) as b:
        explain_all_rows(A, b, A.qs16, [[]] * nq, "DisMax", dis, rows=(257,))
    # a leaf whose only term is absent from segment 1 (the maximum starts at 0.0 there), and one absent from segment 0
    t = A.qs16[1]
    qs = csr([[((int(t[3 * q, 0]), NO_TERM), 1.0), (int(t[3 * q + 1, 0]), 0.5), ((NO_TERM, int(t[3 * q + 2, 0])), -0.75)]
              for q in range(8)], 2)
    absent = dict(q_leaf=np.tile([0, 1, 2], 8), q_plan=np.full(8, 1, np.int32), q_tie=np.full(8, 0.25, F32),
                  q_nleaves=np.full(8, 3, np.uint32))
    with A.ix.prepare(*qs, 257, **absent) as b:
        got, ex = explain_all_rows(A, b, qs, [[]] * 8, "DisMax, absent leaves", absent, rows=(257,))
        assert {0, 1} <= set(got[1][0, :got[3][0]].tolist())


def test_the_edges_of_the_search(Bw):
    """lists of df 1, 64, 65, 4096 and 6000: docs 0 and 5999 are the first and last postings of three of them, doc
    4321 the only posting of one; all three are explained rows of every query"""
    T = Bw.T
    qs = csr([[(T["all"], 1.0), (T["top"], 5.0), (T[name], 0.5 + 0.25 * i)] for i, name in enumerate(("one", "d64", "d65", "d4096"))]
             + [[(T["top"], 2.0), (T["d4096"], 1.0), (T["d64"], 1.5), (T["d65"], 0.75), (T["one"], 3.0), (T["all"], 0.125)]], 1)
    for k in (11, 1025):
        with Bw.ix.prepare(*qs, k) as b:
            got, ex = explain_all_rows(Bw, b, qs, [[]] * 5, f"edges k={k}", rows=(3, 1024) if k == 1025 else (11,))
            for q in range(5):
                assert set(got[0][q, :3].tolist()) == {0, 4321, 5999}


# ---------------------------------------------------------------------------------------------- score stages
def every_kind(Wd):
    """per function kind one that gives some docs a value and some none (a filter, a doc without a value of `pop`, a
    segment without `half`, an infinite `missing`)"""
    lean = [W(2.5), W(-1.5, filter=Wd.flt["f0"]), on(FVF(0, modifier="sqrt", factor=0.5, missing=float("inf")), Wd, "pop"),
            on(FVF(0, modifier="reciprocal"), Wd, "half"), on(FVF(0, modifier="none", missing=3.0), Wd, "half"),
            on(DECAY(0, origin=2500.0, scale=3000.0, offset=100.0, decay=0.5, function="linear"), Wd, "age"),
            on(DECAY(0, origin=5.0, scale=4.0, decay=0.25, function="linear"), Wd, "half")]
    full = [on(POP[0], Wd, "pop"), on(POP[4], Wd, "pop"), on(POP[8], Wd, "pop"), on(AGE[0], Wd, "age"), on(AGE[4], Wd, "age"),
            dict(on(AGE[1], Wd, "age"), filter=Wd.flt["f0"])]
    return lean, full


@pytest.mark.parametrize("k", KS)
def test_every_function_kind_lean_and_full(A, k):
    lean, full = every_kind(A)
    modes = [("sum", "multiply"), ("multiply", "sum"), ("max", "replace"), ("min", "max"), ("avg", "min")]
    for name, fns in (("lean", lean), ("full", lean[:2] + full)):
        specs = [None if q % 5 == 4 else dict(functions=fns[q % 3:] + fns[:q % 3], score_mode=modes[q % 5][0],
                                              boost_mode=modes[q % 5][1], boost=1.0 + 0.25 * (q % 3)) for q in range(16)]
        specs[6] = dict(functions=[], boost=1.0)  # no work: nothing is appended, the score stays
        assert not fscore_ref.unsafe_draws(specs, A.cols)
        chains = [[("fscore", s)] for s in specs]
        with A.ix.prepare(*A.qs16, k, fscore=specs) as b:
            assert b.info()["fscore_kernel"] == name
            got, ex = explain_all_rows(A, b, A.qs16, chains, f"{name} k={k}", rows=(1, 256, 1024) if k == 1025 else (k,))
            nf = ex["n_functions"]
            assert not nf[4].any() and not nf[6].any()            # queries without a spec / without work
            if k > 11:
                assert nf[0].max() == len(specs[0]["functions"])  # some doc has every value ...
                assert nf[0, :got[3][0]].min() < nf[0].max()      # ... and some doc lacks one
        kinds = {X.function_type(f) for f in specs[0]["functions"]}
        assert kinds >= ({"weight", "field_value_factor", "decay_linear"} if name == "lean" else
                         {"weight", "field_value_factor", "decay_exp", "decay_gauss"})


def test_eight_functions_and_a_script_in_both_orders(A):
    """9 entries: the function entries then the script entry (outer), the script entry then the function entries"""
    fns = [W(1.5), W(0.5), on(FVF(0, modifier="none", missing=1.0), A, "pop"), W(2.0), on(FVF(0, modifier="sqrt"), A, "age"),
           W(-0.25), on(DECAY(0, origin=2500.0, scale=5000.0, decay=0.5, function="linear"), A, "age"), W(3.0)]
    specs = [dict(functions=fns, score_mode="sum", boost_mode="sum") if q % 4 != 3 else None for q in range(16)]
    scripts = [A.script("_score * 0.5 + pop / (age + 1)", boost=1.25) if q % 3 != 2 else None for q in range(16)]
    for order in ("outer", "inner"):
        chains = A.chains(scripts, specs, order)
        with A.ix.prepare(*A.qs16, 257, fscore=specs, script=scripts, script_order=order) as b:
            got, ex = explain_all_rows(A, b, A.qs16, chains, f"nine entries, {order}", rows=(257,))
            nf, ty = ex["n_functions"], ex["fn_type"]
            assert (nf[0, :got[3][0]] == 9).all() and (nf[2, :got[3][2]] == 8).all() and (nf[3, :got[3][3]] == 1).all()
            assert not nf[11].any() and got[3][11] > 0  # neither a spec nor a script
            at = 8 if order == "outer" else 0
            assert (ty[0, :got[3][0], at] == N.EXPLAIN_SCRIPT_SCORE).all()
            fields = ex["fn_field"][0, 0].tolist()
            fn_fields = [-1, -1, A.F["pop"], -1, A.F["age"], -1, A.F["age"], -1]
            assert fields == (fn_fields + [-1] if order == "outer" else [-1] + fn_fields)
    shaped = E.shape(ex, {v: n for n, v in A.F.items()}, counts=got[3])
    assert [f.get("field") for f in shaped[0][0]["functions"]] == [None, None, None, "pop", None, "age", None, "age", None]
    assert shaped[0][0]["functions"][0]["type"] == "script_score" and len(shaped[11][0]["functions"]) == 0


def test_rows_that_survive_a_min_score_cut_and_the_eff_rule(A):
    cands = candidates(A, A.qs16, None)
    specs = []
    for q in range(16):
        sc = np.sort(cands[2][q, :cands[3][q]])
        specs.append(dict(functions=[W(2.0), on(FVF(0, modifier="none", missing=1.0), A, "half")], score_mode="multiply",
                          boost_mode="multiply", min_score=float(2.0 * sc[len(sc) // 2]), max_boost=float(40.0 * sc[-1])))
    with A.ix.prepare(*A.qs16, 1025, fscore=specs) as b:
        got, ex = explain_all_rows(A, b, A.qs16, [[("fscore", s)] for s in specs], "min_score", rows=(1024,))
        assert (got[3] < cands[3]).all() and (got[3] > 0).all()  # the cut dropped docs, and rows survived it
    # a first pass that scores 0.0 (weight 0): base_score stays 0.0, the functions still count
    qs = (A.qs16[0], A.qs16[1], np.zeros_like(A.qs16[2]))
    spec = [dict(functions=[W(4.0)], score_mode="sum", boost_mode="multiply")] * 16
    with A.ix.prepare(*qs, 11, fscore=spec) as b:
        got, ex = explain_all_rows(A, b, qs, [[("fscore", s)] for s in spec], "zero base", rows=(11,))
        assert not ex["base_score"].any() and (ex["final_score"] == 4.0).all()


# ---------------------------------------------------------------------------------------------- compound requests
def test_function_score_under_a_field_sort_and_a_cursor_batch(A):
    rng = np.random.default_rng(41)
    vals = [[[int(rng.integers(0, 8))] for _ in range(s.n_docs)] for s in A.segs]
    fid = A.ix.add_sort_field(vals, np.int64)
    specs = [dict(functions=[W(1.5), on(FVF(0, modifier="sqrt"), A, "pop")], score_mode="sum", boost_mode="sum")] * 16
    chains = [[("fscore", s)] for s in specs]
    try:
        with A.ix.prepare_request(*A.qs16, 257, sort=[(fid, "asc"), ("_score", "desc")], fscore=specs) as b:
            got, _ = explain_all_rows(A, b, A.qs16, chains, "field sort", rows=(257,))
            assert (np.diff(got[2][0, :got[3][0]]) > 0).any()  # not in score order
    finally:
        A.ix.remove_sort_field(fid)
    with A.ix.prepare_request(*A.qs16, 11, fscore=specs) as b:
        first, _ = explain_all_rows(A, b, A.qs16, chains, "first page", rows=(11,))
    cursors = [((float(first[2][q, 4]),), int(first[1][q, 4]), int(first[0][q, 4])) if q % 2 == 0 else None for q in range(16)]
    with A.ix.prepare_request(*A.qs16, 11, cursors=cursors, fscore=specs) as b:
        page, ex = explain_all_rows(A, b, A.qs16, chains, "cursor page", rows=(11,))
        assert np.array_equal(page[0][0, :6], first[0][0, 5:11]) and np.array_equal(page[0][1], first[0][1])


def test_a_bool_clause_stage_and_function_score(A):
    t = A.qs16[1]
    queries = [([(MUST, [int(t[3 * q, 0])]), (MUST_NOT, [int(t[3 * q + 2, 0])])], 0) if q % 2 else
               ([(SHOULD, [int(t[3 * q + 1, 0])]), (SHOULD, [int(t[3 * q + 2, 0])])], 1) for q in range(16)]
    cl = bool_ref.clauses_of(queries, 2)
    specs = [dict(functions=[on(FVF(0, modifier="reciprocal"), A, "half"), W(0.5, filter=A.flt["f0"])], score_mode="sum",
                  boost_mode="multiply", boost=2.0)] * 16
    plain = A.ix.search_plan(*A.qs16, 257)
    with A.ix.prepare_request(*A.qs16, 257, clauses=cl, fscore=specs) as b:
        got, ex = explain_all_rows(A, b, A.qs16, [[("fscore", s)] for s in specs], "bool + function_score", rows=(257,))
        assert (got[3] <= plain[3]).all() and (got[3] < plain[3]).any() and (got[3] > 0).any()  # the clauses rejected docs


@pytest.mark.parametrize("k", KS)
def test_a_rescore_batch(A, k):
    """matched rows, unmatched rows and rows behind the window: base is the first-pass score computed again — the
    oracle's, and first_score of slg_batch_fetch_rescore — final the row's score, the rescore part the batch's own"""
    rng = np.random.default_rng(43)
    rq = [[(int(a), float(F32(0.5 + 0.25 * i))) for i, a in enumerate(rng.choice(40, size=2, replace=False))] for _ in range(16)]
    rq[3] = []  # a rescore query without a term: nothing is rescored
    window = {11: 5, 257: 40, 1025: 64}[k]
    rescore = dict(zip(("q_offsets", "q_terms", "q_weights"), csr(rq, 2)), window=window, mode=rescore_ref.MULTIPLY)
    want = rescore_ref.reference(A.oracle, A.segs, *A.qs16, k, rescore)
    with A.ix.prepare_request(*A.qs16, k, rescore=rescore) as b:
        b.run()
        got = b.fetch() + b.rescore_details()
        same(got, want, f"rescore k={k}")
        look = X.base_lookup(candidates(A, A.qs16, None))
        for rows in (1, 256, 1024):
            ex = b.explain(rows)
            n = [min(rows, int(got[3][q])) for q in range(16)]
            per_q = [X.explain_rescore((got[0][q], got[1][q], got[2][q], got[4][q], got[5][q], got[6][q]), n[q]) for q in range(16)]
            arrays = X.as_arrays(per_q, rows, with_rescore=True)
            assert sorted(ex) == sorted(arrays)
            for name in arrays:
                assert np.array_equal(bits(ex[name]), bits(arrays[name])), (name, rows)
            for q in range(16):  # ... and the base is the oracle's first-pass score of the doc
                base = [look[q][(int(got[1][q, i]), int(got[0][q, i]))] for i in range(n[q])]
                assert np.array_equal(bits(ex["base_score"][q, :n[q]]), bits(np.array(base, F32))), q
        flag, cnt = got[6], got[3]
        assert not ex["n_functions"].any() and not flag[3].any()
        if k > 11:  # some query has all three kinds of row: matched, unmatched, behind the window
            assert any(flag[q, :window].any() and not flag[q, :window].all() and cnt[q] > window for q in range(16))
        shaped = E.shape(ex, {}, counts=cnt)
        assert all(("rescore" in h) == bool(flag[q, i]) for q in range(16) for i, h in enumerate(shaped[q]))


# ---------------------------------------------------------------------------------------------- lifecycle
def test_explain_twice_and_two_batches_in_flight(A, Bw):
    import torch
    specs = [dict(functions=[W(2.0), on(FVF(0, modifier="sqrt"), A, "pop")], score_mode="sum", boost_mode="sum")] * 16
    chains = [[("fscore", s)] for s in specs]
    with A.ix.prepare(*A.qs16, 257, fscore=specs) as b:
        b.run()
        _, one = check(A, b, A.qs16, chains, 257, "first call")
        _, two = check(A, b, A.qs16, chains, 257, "second call")
        assert all(np.array_equal(bits(one[n]), bits(two[n])) for n in one)
        b.run()  # and a second run of the batch leaves the rows explainable
        check(A, b, A.qs16, chains, 11, "after a second run")
    T = Bw.T
    qs = csr([[(T["all"], 1.0), (T["top"], 5.0), (T["d64"], 0.5)], [(T["all"], 1.0), (T["d4096"], 0.5)]], 1)
    fs = [[dict(functions=[on(FVF(0, modifier="sqrt"), Bw, "rank")], boost_mode="sum")] * 2,
          [dict(functions=[W(3.0), on(FVF(0, modifier="none", factor=0.001), Bw, "rank")], score_mode="sum", boost_mode="sum")] * 2]
    streams = [torch.cuda.Stream() for _ in fs]
    batches = [Bw.ix.prepare(*qs, 1025, fscore=f) for f in fs]
    for bb, s in zip(batches, streams):
        bb.set_stream(s.cuda_stream)
    for _ in range(2):
        for bb in batches:
            bb.run()
    for bb, f in zip(batches, fs):
        check(Bw, bb, qs, [[("fscore", s)] for s in f], 1024, "in flight")
        bb.close()


def test_a_batch_prepared_before_an_update_is_explained_against_its_state(oracle):
    import searchlite_amd as sa
    rng = np.random.default_rng(47)
    segs = [random_segment(rng, 300, 30, 6), random_segment(rng, 200, 30, 6)]
    qs = random_queries(rng, 8, 3, 30, n_segs=2, weights=True)
    old = fscore_ref.all_candidates(oracle, segs, *qs)
    want_rows = oracle.search_batch(segs, *qs, 33, strategy=oracle.BM25)
    with sa.GpuIndex(segs, tuning={"updatable": 1}) as ix:
        b = ix.prepare(*qs, 33)
        bm = dead_bitmap(rng, 300, 0.3)
        ix.update_deleted(0, bm, 300.0 - float(np.unpackbits(bm, bitorder="little")[:300].sum()))
        b.run()
        got = b.fetch()
        same(got, want_rows, "prepared before the update")
        ex = b.explain(33)
        look = X.base_lookup(old)  # the impacts of the state the batch was prepared on (idf follows live_docs)
        for q in range(8):
            base = np.array([look[q][(int(got[1][q, i]), int(got[0][q, i]))] for i in range(int(got[3][q]))], F32)
            assert np.array_equal(bits(ex["base_score"][q, :len(base)]), bits(base))
        assert np.array_equal(bits(ex["final_score"]), bits(got[2]))
        b.close()
        with ix.prepare(*qs, 33) as b2:  # and a batch prepared after it against the new one
            b2.run()
            new = fscore_ref.all_candidates(oracle, ix.segments, *qs)
            got2, ex2 = b2.fetch(), b2.explain(33)
            look = X.base_lookup(new)
            for q in range(8):
                base = np.array([look[q][(int(got2[1][q, i]), int(got2[0][q, i]))] for i in range(int(got2[3][q]))], F32)
                assert np.array_equal(bits(ex2["base_score"][q, :len(base)]), bits(base))
            assert not np.array_equal(bits(ex2["base_score"]), bits(ex["base_score"]))


def test_refusals_that_need_a_device(A):
    def refused(b, rows, code, what):
        with pytest.raises(N.SlgError) as ei:
            b.explain(rows)
        assert ei.value.code == code and what in str(ei.value), str(ei.value)

    with A.ix.prepare(*A.qs16, 11) as b:
        refused(b, 11, N.ERR_INVALID, "has not run")
        b.run()
        refused(b, 0, N.ERR_INVALID, "rows is 0")
        refused(b, 1025, N.ERR_UNSUPPORTED, "SLG_MAX_EXPLAIN_ROWS")
        assert b.explain(1024)["base_score"].shape == (16, 1024)
    with A.ix.prepare_scan([{"match_all": {}}, {"constant_score": {"boost": 2.0}}], 11) as b:
        b.run()
        refused(b, 11, N.ERR_UNSUPPORTED, "scan batch")
    nq = 16
    two = dict(q_nleaves=np.full(nq, 3, np.uint32), q_plan=np.zeros(nq, np.int32),
               q_leaf_offsets=(np.arange(nq + 1) * 3).astype(np.uint32), leaf_group=np.tile(np.array([0, 0, 1], np.uint32), nq),
               q_group_offsets=(np.arange(nq + 1) * 2).astype(np.uint32), group_plan=np.tile(np.array([1, 0], np.int32), nq),
               group_tie=np.tile(np.array([0.3, 0.0], F32), nq))
    with A.ix.prepare(*A.qs16, 11, **two) as b:
        b.run()
        refused(b, 11, N.ERR_UNSUPPORTED, "two-level or deeper score plan")
