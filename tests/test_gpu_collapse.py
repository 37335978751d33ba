"""Field collapsing on the device (slg_batch_prepare_collapse / slg_batch_fetch_collapse).

Expected: the oracle run with k >= the number of docs gives every accepted doc with its exact score; those hits in
the batch's order (score order as they are, a field sort by the restated SortKey of tests/collapse_ref.py), cut at
k or paged behind a cursor, are the batch's rows, and tests/collapse_ref.py — collapse_hits restated, itself checked
against hand-derived tables in tests/test_collapse_ref.py — collapses them.  Bar: every array equal, integers as they
are and scores as f32 bit patterns, zeros past the counts; the rows of a collapse batch equal the same batch without
the spec bit for bit.  The world and what it must provide: tests/collapse_world.py, tests/test_collapse_world.py.

The inner slice (from, size) = (600, 1) lies beyond SLG_MAX_INNER_HITS (inner_from + inner_size <= 64, one member per
lane of a wave), which the library must refuse with SLG_ERR_UNSUPPORTED: wherever that slice comes up the case
asserts the refusal, and (63, 1) — the largest `from` the library takes — is the `from >= members` case that runs.
"""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from tests import collapse_ref as R
from tests import collapse_world as CW
from tests.util import load_golden, random_segment

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return sa


def open_world(gpu, w):
    w = dict(w)
    w["ix"] = ix = gpu.GpuIndex(w["segs"])
    w["sort_ids"] = {n: ix.add_sort_field(v, np.float64 if is_f else np.int64) for n, (v, is_f) in w["fields"].items()}
    w["col_ids"] = {n: ix.add_agg_keyword_field(col, n_ords) for n, (col, n_ords) in w["columns"].items()}
    w["rows"] = {}
    return w


@pytest.fixture(scope="module")
def W(gpu, oracle):
    w = open_world(gpu, CW.build(oracle))
    yield w
    w["ix"].close()


def ids_of(sort, ids):
    return None if sort is None else [(p if p == "_score" else ids[p], o) for p, o in sort]


def all_rows(W, main_sort):
    key = repr(main_sort)
    if key not in W["rows"]:
        W["rows"][key] = CW.sorted_rows(W["all"], main_sort, W["fields"])
    return W["rows"][key]


def same_rows(got, want, what):
    for a, b, name in zip(got, want, ("doc", "seg", "score", "count")):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: rows differ in {name}"


def run_case(W, k, column, G, inner=None, inner_sort=None, main_sort=None, after=None, twice=False, what=""):
    """one collapse batch against the reference; inner: None or (from, size); after: None or the rank behind which
    the page starts (a cursor batch); G: a number or "total" (query 0's total_groups, at least 1) -> the arrays"""
    what = f"{what} k={k} col={column} G={G} inner={inner} inner_sort={inner_sort} sort={main_sort} after={after}"
    ix, fields = W["ix"], W["fields"]
    rows = all_rows(W, main_sort)
    cursors = None
    if after is not None:
        cursors, paged = [], []
        for hits in rows:
            if len(hits) < after:
                cursors.append(None)
                paged.append(hits)
                continue
            s, d, sc = hits[after - 1]
            parts = main_sort or R.SCORE_DESC
            vals = tuple(float(sc) if p == "_score" else R.pick(fields[p][0][s][d], o) for p, o in parts)
            cursors.append((vals, s, d))
            paged.append(hits[after:])
        rows = paged
    want_rows = CW.as_arrays(rows, k)
    col = W["columns"][column][0]
    frm, size = inner or (0, 0)
    expect = lambda g: R.expected_arrays(*want_rows, col, g, frm, size, inner_sort, main_sort, fields)
    if G == "total":
        G = min(max(int(expect(1)["total_groups"][0]), 1), k)
    want = expect(G)
    q = (W["offs"], W["terms"], W["w"])
    spec = dict(field=W["col_ids"][column], group_limit=G, inner_from=frm, inner_size=size,
                inner_sort=ids_of(inner_sort, W["sort_ids"]))
    kw = dict(sort=ids_of(main_sort, W["sort_ids"]), cursors=cursors)
    if size > 0 and frm + size > CW.MAX_INNER_HITS:  # not built: refused for the CPU path, nothing runs
        from searchlite_amd import _native as N
        with pytest.raises(N.SlgError) as ei:
            ix.prepare(*q, k, collapse=spec, **kw)
        assert ei.value.code == N.ERR_UNSUPPORTED and "SLG_MAX_INNER_HITS" in ei.value.msg, what
        return None
    with ix.prepare(*q, k, collapse=spec, **kw) as b:
        b.run()
        got_rows, got = b.fetch(), b.collapse_groups()
        if twice:
            b.run()
            again_rows, again = b.fetch(), b.collapse_groups()
            same_rows(again_rows, got_rows, what + " second run")
            R.assert_same_arrays(again, got, what + " second run")
    same_rows(got_rows, want_rows, what + " vs the oracle")
    with ix.prepare(*q, k, **kw) as plain:
        plain.run()
        same_rows(got_rows, plain.fetch(), what + " vs the batch without collapse")
    R.assert_same_arrays(got, want, what)
    return got


COLUMNS = ("seven", "one", "own", "big", "noseg", "multi")


@pytest.mark.parametrize("k", CW.KS)
def test_every_column_at_every_k(W, k):
    """score order; every column with G in {1, query 0's total, k}, the inner hits' (from, size) rotating so that
    every pair meets every k, every column and every kind of G"""
    ki = CW.KS.index(k)
    for ci, column in enumerate(COLUMNS):
        for gi, G in enumerate((1, "total", k)):
            got = run_case(W, k, column, G, CW.INNERS[(ki + ci + gi) % len(CW.INNERS)], twice=(gi == 1 and ci == ki % 6))
            if column == "multi" and got is not None:  # status 1 exactly where the reference fails, and nothing else but zeros there
                bad = got["status"] == 1
                assert not any(v[bad].any() for n, v in got.items() if n != "status")


@pytest.mark.parametrize("inner", CW.INNERS)
def test_every_inner_slice(W, inner):
    for k in (65, 620):
        for G in (1, "total", k):
            run_case(W, k, "seven", G, inner)
            run_case(W, k, "seven", G, inner, [("low", "asc")])


@pytest.mark.parametrize("inner_sort", [[("low", "asc")], [("_score", "asc")], [("f64", "desc")],
                                        [("f64", "desc"), ("low", "asc"), ("_score", "asc"), ("low", "desc")],
                                        [("_score", "desc")], []], ids=repr)
def test_inner_sorts_in_score_order(W, inner_sort):
    """ties of `low` fall to (segment, doc), not to row order; `_score` desc and an empty sort are the batch's own
    order; the one-ordinal column puts > 64 members into one group, so the wave reads more than one chunk"""
    for k in (64, 257, 620):
        run_case(W, k, "seven", 7, (0, 64), inner_sort)
        run_case(W, k, "one", 1, (3, 61), inner_sort)
        run_case(W, k, "big", k, (1, 2), inner_sort)
    got = run_case(W, 620, "one", 1, (0, 64), inner_sort)
    assert got["group_size"][0, 0] > 129 and got["inner_count"][0, 0] == 64


def test_field_sorted_batches(W):
    main = [("low", "asc")]
    for k in (11, 257):
        null = run_case(W, k, "seven", 5, (0, 3), None, main)
        given = run_case(W, k, "seven", 5, (0, 3), main, main)
        R.assert_same_arrays(given, null, "inner sort equal to the batch's")
        by_score = run_case(W, k, "seven", 5, (0, 3), [("_score", "desc")], main)  # all scores 0.0: (segment, doc)
        assert not by_score["inner_score"].view(np.uint32).any() and not by_score["group_score"].view(np.uint32).any()
        run_case(W, k, "seven", 5, (0, 3), [], main)
        run_case(W, k, "one", 1, (2, 62), [("f64", "desc"), ("_score", "desc")], [("low", "asc"), ("_score", "desc")])
    assert not np.array_equal(by_score["inner_row"], null["inner_row"])


def test_cursor_batches(W):
    for main in (None, [("low", "asc")]):
        for k in (11, 65):
            run_case(W, k, "seven", 5, (0, 3), None, main, after=5)
            run_case(W, k, "seven", 5, (1, 2), [("f64", "desc")], main, after=5, twice=True)
            run_case(W, k, "multi", k, None, None, main, after=5)


def test_k_4096(gpu, oracle):
    """a fourth segment of 5000 docs: query 0 fills all 4096 rows"""
    from searchlite_amd import _native as N
    w = open_world(gpu, CW.build(oracle, big=True))
    try:
        assert int(w["all"][3][0]) > 4096
        k = N.MAX_COLLAPSE_ROWS
        got = run_case(w, k, "seven", 10, (0, 3), [("low", "asc")], twice=True)
        assert got["group_size"][0].sum() > 3000
        run_case(w, k, "own", k, (0, 1))
        run_case(w, k, "big", 10, (2, 3), None, [("low", "asc")])
        spec = dict(field=w["col_ids"]["seven"], group_limit=10)
        with pytest.raises(N.SlgError) as ei:
            w["ix"].prepare(w["offs"], w["terms"], w["w"], k + 1, collapse=spec)
        assert ei.value.code == N.ERR_UNSUPPORTED and "SLG_MAX_COLLAPSE_ROWS" in ei.value.msg
    finally:
        w["ix"].close()


def test_one_call_form(W):
    from searchlite_amd import _native as N
    from searchlite_amd.searcher import collapse_spec, sort_spec
    ix, k, G, S = W["ix"], 65, 4, 2
    spec, keep = collapse_spec(dict(field=W["col_ids"]["seven"], group_limit=G, inner_from=1, inner_size=S,
                                    inner_sort=[(W["sort_ids"]["low"], "asc")]))
    main = sort_spec([(W["sort_ids"]["f64"], "desc")])
    nq = 16
    shapes = [(nq, k)] * 3 + [(nq,)] * 4 + [(nq, G)] * 7 + [(nq, G, S)] * 4
    f32 = {2, 12, 17}
    outs = [np.zeros(s, np.float32 if i in f32 else np.uint32) for i, s in enumerate(shapes)]
    o, t, w = W["offs"], np.ascontiguousarray(W["terms"]), W["w"]
    N.check(ix._lib.slg_search_batch_collapse(ix._h, nq, o.ctypes.data, t.ctypes.data, w.ctypes.data, None, None,
                                              C.addressof(main), None, C.addressof(spec), k, 1,
                                              *[a.ctypes.data for a in outs]))
    got = run_case(W, k, "seven", G, (1, S), [("low", "asc")], [("f64", "desc")])
    names = ("n_groups total_groups status group_row group_ord group_size group_doc group_seg group_score "
             "inner_count inner_row inner_doc inner_seg inner_score").split()
    R.assert_same_arrays(dict(zip(names, outs[4:])), got, "one call")
    same_rows(tuple(outs[:4]), CW.as_arrays(all_rows(W, [("f64", "desc")]), k), "one call")
    # every output pointer may be NULL
    with ix.prepare(o, t, w, k, collapse=(spec, keep)) as b:
        b.run()
        N.check(ix._lib.slg_batch_fetch_collapse(b._h, *[None] * 14))


def test_lifecycle_and_errors(gpu, oracle, W):
    from searchlite_amd import _native as N
    from searchlite_amd import searcher
    q = (W["offs"], W["terms"], W["w"])
    with gpu.GpuIndex([copy.copy(s) for s in W["segs"]]) as ix:
        col, n_ords = W["columns"]["seven"]
        fid = ix.add_agg_keyword_field(col, n_ords)
        num = ix.add_agg_field([[[1.5]] * n for n in W["n_docs"]], np.float64)
        low = ix.add_sort_field(W["fields"]["low"][0], np.int64)
        spec = dict(field=fid, group_limit=5, inner_from=0, inner_size=2, inner_sort=[(low, "asc")])
        want = R.expected_arrays(*CW.as_arrays(all_rows(W, None), 65), col, 5, 0, 2, [("low", "asc")], None, W["fields"])

        def refused(code, word, **over):
            with pytest.raises(N.SlgError) as ei:
                ix.prepare(*q, 65, collapse=dict(spec, **over))
            assert ei.value.code == code and word in ei.value.msg, ei.value.msg
        refused(N.ERR_INVALID, "unknown agg field", field=fid + 100)
        refused(N.ERR_INVALID, "numeric", field=num)
        refused(N.ERR_INVALID, "unknown sort field", inner_sort=[(low + 100, "asc")])
        refused(N.ERR_INVALID, "group_limit", group_limit=66)
        refused(N.ERR_UNSUPPORTED, "SLG_MAX_INNER_HITS", inner_from=63)

        b = ix.prepare(*q, 65, collapse=spec)
        plain = ix.prepare(*q, 65)
        try:
            with pytest.raises(N.SlgError) as ei:  # before the run
                b.collapse_groups()
            assert ei.value.code == N.ERR_INVALID and "has not run" in ei.value.msg
            plain.run()
            assert ix._lib.slg_batch_fetch_collapse(plain._h, *[None] * 14) == N.ERR_INVALID  # another kind of batch
            assert b"not a collapse batch" in ix._lib.slg_last_error()
            group = searcher.ShardGroup(ix, 0, 1, searcher.shard_unique_id(), len(W["segs"]))
            try:
                for call in (lambda: b.run_sharded(group), lambda: b.run_sharded(group, fetch=False, seq=0),
                             b.fetch_sharded):
                    with pytest.raises(N.SlgError) as ei:
                        call()
                    assert ei.value.code == N.ERR_UNSUPPORTED and "collapse" in ei.value.msg
            finally:
                group.close()
            # the batch keeps the columns of the state it was prepared on
            ix.remove_agg_field(fid)
            ix.remove_sort_field(low)
            b.run()
            R.assert_same_arrays(b.collapse_groups(), want, "after remove_agg_field")
            refused(N.ERR_INVALID, "unknown agg field")
        finally:
            b.close()
            plain.close()
        # a segment added after the column was registered has none: the field must be registered again
        fid2 = ix.add_agg_keyword_field(col, n_ords)
        ix.add_segment(random_segment(np.random.default_rng(5), 50, 40, 25, k1=0.9, b=0.4))
        terms4 = np.ascontiguousarray(np.concatenate([W["terms"], np.full_like(W["terms"][:, :1], CW.NO_TERM)], axis=1))
        with pytest.raises(N.SlgError) as ei:
            ix.prepare(W["offs"], terms4, W["w"], 65, collapse=dict(field=fid2, group_limit=5))
        assert ei.value.code == N.ERR_INVALID and "no column for segment 3" in ei.value.msg
        fid3 = ix.add_agg_keyword_field(col + [None], n_ords)
        with ix.prepare(W["offs"], terms4, W["w"], 65, collapse=dict(field=fid3, group_limit=5)) as b3:
            b3.run()
            got = b3.collapse_groups()
        for name in ("n_groups", "total_groups", "group_row", "group_ord", "group_size"):
            assert np.array_equal(got[name], want[name]), name


def test_inner_sort_field_predates_the_added_segment(gpu, W):
    """the world of the added-segment case above (the three segments, then one of 50 docs that holds no query term),
    queries 0 .. 3: an inner sort over a sort field registered before the fourth segment is refused, as the column
    is; over the field registered again the arrays are the reference's for the rows, which all lie in the first three
    segments"""
    from searchlite_amd import _native as N
    nq, k = 4, 65
    offs = W["offs"][:nq + 1]
    terms4 = np.concatenate([W["terms"], np.full_like(W["terms"][:, :1], CW.NO_TERM)], axis=1)
    q = (offs, np.ascontiguousarray(terms4[:offs[nq]]), W["w"][:offs[nq]])
    col, n_ords = W["columns"]["seven"]
    low = W["fields"]["low"][0]
    want = R.expected_arrays(*CW.as_arrays(all_rows(W, None)[:nq], k), col, 5, 0, 2, [("low", "asc")], None, W["fields"])
    with gpu.GpuIndex([copy.copy(s) for s in W["segs"]]) as ix:
        before = ix.add_sort_field(low, np.int64)
        ix.add_segment(random_segment(np.random.default_rng(5), 50, 40, 25, k1=0.9, b=0.4))
        spec = dict(field=ix.add_agg_keyword_field(col + [None], n_ords), group_limit=5, inner_from=0, inner_size=2)
        with pytest.raises(N.SlgError) as ei:
            ix.prepare(*q, k, collapse=dict(spec, inner_sort=[(before, "asc")]))
        assert ei.value.code == N.ERR_INVALID, ei.value.msg
        assert "collapse: sort field" in ei.value.msg and "no column for segment" in ei.value.msg, ei.value.msg
        again = ix.add_sort_field(low + [[[0]] * 50], np.int64)
        with ix.prepare(*q, k, collapse=dict(spec, inner_sort=[(again, "asc")])) as b:
            b.run()
            R.assert_same_arrays(b.collapse_groups(), want, "inner sort over the field registered again")


def test_recipes_collapse_quick_by_cuisine(gpu, oracle):
    """recipes/queries/collapse-quick-by-cuisine.json as far as this library goes: the golden queries of
    recipes.npz under `total_time_minutes` asc, collapsed on `cuisine` (28 keys, every doc single-valued), limit 5
    (k = limit + 1 = 6) and a candidate window of 100 (k = 101), inner_hits {size 2, sort total_time_minutes asc}"""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    segs, z = load_golden("recipes.npz")
    srt, cz = np.load(os.path.join(here, "recipes_sort.npz")), np.load(os.path.join(here, "recipes_collapse.npz"))
    offs, vals = srt["total_time_minutes_offsets"], srt["total_time_minutes"]
    c_offs, c_ords = cz["cuisine_offsets"], cz["cuisine_ords"]
    n = segs[0].n_docs
    assert len(cz["cuisine_keys"]) == 28 and len(c_offs) == n + 1 and (np.diff(c_offs) == 1).all()
    fields = {"ttm": ([[[int(v) for v in vals[offs[d]:offs[d + 1]]] for d in range(n)]], False)}
    column = [[[int(o) for o in c_ords[c_offs[d]:c_offs[d + 1]]] for d in range(n)]]
    qo, qt, qw = z["q_offsets"], z["q_terms"], z["q_weights"]
    main = [("ttm", "asc")]
    rows = CW.sorted_rows(oracle.search_batch(segs, qo, qt, qw, n, strategy=oracle.WAND), main, fields)
    with gpu.GpuIndex(segs) as ix:
        sid = ix.add_sort_field([(offs, vals)], np.int64)
        cid = ix.add_agg_keyword_field([(c_offs, c_ords)], 28)
        for k in (6, 101):
            want_rows = CW.as_arrays(rows, k)
            want = R.expected_arrays(*want_rows, column, 5, 0, 2, main, main, fields)
            doc, seg, score, count, got = ix.search_collapse(
                qo, qt, qw, k, dict(field=cid, group_limit=5, inner_size=2, inner_sort=[(sid, "asc")]), sort=[(sid, "asc")])
            same_rows((doc, seg, score, count), want_rows, f"recipes k={k}")
            R.assert_same_arrays(got, want, f"recipes k={k}")
        assert (want["total_groups"] > 5).any() and want["inner_count"].any()
