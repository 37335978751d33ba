"""The two per-query radix-select kernels (select_topk_kernel, select_sorted_kernel; slg_kernels.hpp) at their
range, slice-table and tie edges, through search_plan, search_sorted, search_after and search_batch_bool.

Tolerance 0: the same (segment, doc) sequence, score bits, counts, matched and seen as the oracle, zero rows past the
count.  Score order is the oracle at the same k; sorts and cursors are the oracle at k >= docs ordered by the
restatements of SortKey::cmp in tests/test_gpu_sort.py and tests/test_gpu_cursor.py.  The worlds are those of
tests/select_edge_worlds.py; tests/test_select_edges_worlds.py proves on the CPU that every query has the candidate
count, ties, slice count and region pattern its case needs."""
import numpy as np
import pytest

from tests import bool_ref as B
from tests import select_edge_worlds as SW
from tests.test_gpu_bool import same
from tests.test_gpu_cursor import check_row, cursor_of, ordered_rows
from tests.test_gpu_sort import check as check_sorted, expected_rows

pytestmark = pytest.mark.gpu

SPECS = {
    "four_score_last": [("low", "desc"), ("f64", "asc"), ("i64", "asc"), ("_score", "asc")],
    "low_score_last": [("low", "asc"), ("_score", "desc")],
    "match_only": [("i64", "desc")],
}


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return sa


class Dev:
    """an index over a world under one tuning, with the world's sort fields and one doc filter"""

    def __init__(self, sa, W, tuning):
        self.W = W
        self.ix = sa.GpuIndex(W.segs, tuning=tuning)
        self.ids = {nm: self.ix.add_sort_field(v, np.float64 if is_f else np.int64) for nm, (v, is_f) in W.fields.items()}
        self.masks = W.masks(99)
        self.fid = self.ix.add_filter(self.masks)

    def sort(self, spec):
        return None if spec is None else [(p if p == "_score" else self.ids[p], o) for p, o in spec]


_devs, _rows = {}, {}


@pytest.fixture(scope="module")
def dev(gpu):
    """dev(world name, tuning name) -> Dev, built once per module"""
    worlds = {"ranges": SW.ranges_world, "ties": SW.ties_world, "slices": SW.slices_world,
              "ranges_del": lambda: SW.ranges_world().tombstoned(1, 61),
              "slices_del": lambda: SW.slices_world().tombstoned(0, 62)}
    tunings = {"default": {}, "no_seed": SW.NO_SEED, "slice": SW.SLICE_TUNING, "region": SW.REGION_TUNING}

    def get(world, tuning):
        if (world, tuning) not in _devs:
            _devs[(world, tuning)] = Dev(gpu, worlds[world](), tunings[tuning])
        return _devs[(world, tuning)]
    yield get
    for d in _devs.values():
        d.ix.close()
    _devs.clear()


def rows_of(oracle, W, key, names, sort):
    """the full expected order of every query (ordered_rows), computed once per (queries, sort)"""
    ck = (key, None if sort is None else tuple(sort))
    if ck not in _rows:
        hits = oracle.search_batch(W.segs, *W.queries(names), W.k_all, strategy=oracle.BM25)
        _rows[ck] = ordered_rows(hits, None if sort is None else list(sort), W.fields)
    return _rows[ck]


def zero_tail(got, what):
    doc, seg, score, count = got[:4]
    for q in range(len(count)):
        n = int(count[q])
        assert not (doc[q, n:].any() or seg[q, n:].any() or score[q, n:].view(np.uint32).any()), \
            f"{what}: query {q} has rows past its count"


def check_sorted_rows(got, rows, k, sort, what):
    check_sorted(got, [[(h.seg, h.doc, h.score) for h in r] for r in rows], k, sort, what)
    zero_tail(got, what)


def check_after(got, rows, cursors, k, sort, fields, what):
    for q in range(len(rows)):
        check_row(got, q, rows[q], cursors[q], k, sort, fields, what=what)
    zero_tail(got, what)


def with_cursors(W, names, rows, extra, ranks):
    """the queries once without a cursor, then the queries `extra` again with a cursor at each rank of `ranks`"""
    all_names = list(names) + [nm for nm in extra for _ in ranks]
    all_rows = list(rows) + [rows[names.index(nm)] for nm in extra for _ in ranks]
    cursors = [None] * len(names) + [cursor_of(rows[names.index(nm)][r]) for nm in extra for r in ranks]
    return W.queries(all_names), all_rows, cursors


# ---- case 1: the rank ranges of select_topk_kernel -------------------------------------------------------------
@pytest.mark.parametrize("k", SW.TOPK_KS)
def test_topk_range_boundaries(dev, oracle, k):
    """n = k - 1, k, k + 1 and 9 000 candidates, in one segment and over two; without a threshold seed (n exact) and
    at the default tuning; select_topk_kernel<false> (search_plan) and <true> (search_after: no cursor, and a cursor
    at ranks 0, 2047 and 2048 of the full order)"""
    W = SW.ranges_world()
    names = W.topk_names
    qs = W.queries(names)
    want = oracle.search_batch(W.segs, *qs, k, strategy=oracle.BM25)
    assert {k - 1, k, k + 1} <= set(W.n[nm] for nm in names)
    for tuning in ("no_seed", "default"):
        same(dev("ranges", tuning).ix.search_plan(*qs, k), want, f"k={k} {tuning}")
    rows = rows_of(oracle, W, "topk", names, None)
    cq, crows, cursors = with_cursors(W, names, rows, ["b9000", "a6146", "b4097"], (0, 2047, 2048))
    got = dev("ranges", "no_seed").ix.search_after(*cq, k, cursors)
    check_after(got, crows, cursors, k, None, W.fields, f"k={k} after")


# ---- case 2: the rank ranges of select_sorted_kernel -----------------------------------------------------------
@pytest.mark.parametrize("k", SW.SORTED_KS)
@pytest.mark.parametrize("spec", list(SPECS))
def test_sorted_range_boundaries(dev, oracle, spec, k):
    """the same n pattern around kSortedCap = 1 024; select_sorted_kernel<false> (search_sorted) and <true>
    (search_after with the sort: no cursor, and a cursor at ranks 0, 1023 and 1024)"""
    W, D = SW.ranges_world(), dev("ranges", "no_seed")
    names, sort = W.sorted_names, SPECS[spec]
    assert {k - 1, k, k + 1} <= set(W.n[nm] for nm in names)
    rows = rows_of(oracle, W, "sorted", names, sort)
    check_sorted_rows(D.ix.search_sorted(*W.queries(names), k, D.sort(sort)), rows, k, sort, f"{spec} k={k}")
    cq, crows, cursors = with_cursors(W, names, rows, ["b9000", "a3074"], (0, 1023, 1024))
    got = D.ix.search_after(*cq, k, cursors, sort=D.sort(sort))
    check_after(got, crows, cursors, k, sort, W.fields, f"{spec} k={k} after")


def test_sorted_expected_rows_agree(oracle):
    """the two restatements of SortKey::cmp give one order (expected_rows is the reference of a sorted batch)"""
    W = SW.ranges_world()
    hits = oracle.search_batch(W.segs, *W.queries(W.sorted_names[:6]), W.k_all, strategy=oracle.BM25)
    for spec, sort in SPECS.items():
        a = expected_rows(hits, sort, W.fields)
        b = ordered_rows(hits, sort, W.fields)
        assert [[(h[0], h[1]) for h in r] for r in a] == [[(h.seg, h.doc) for h in r] for r in b], spec


# ---- case 3: ties that only segment and doc resolve, across range boundaries --------------------------------
@pytest.mark.parametrize("k", [2049, 4097, 6145])
def test_topk_ties_across_ranges(dev, oracle, k):
    """6 145 candidates of one score over two segments: the select descends to the last byte of the doc word"""
    W, D = SW.ties_world(), dev("ties", "no_seed")
    qs = W.queries(["tie_topk", "tie_x", "tie_y"])
    want = oracle.search_batch(W.segs, *qs, k, strategy=oracle.BM25)
    cap = SW.SELECT_CAP
    assert want[2][0, cap - 1].view(np.uint32) == want[2][0, cap].view(np.uint32)
    same(D.ix.search_plan(*qs, k), want, f"ties k={k}")
    rows = rows_of(oracle, W, "ties", ["tie_topk", "tie_x", "tie_y"], None)
    cursors = [None, None, cursor_of(rows[2][cap // 2])]
    check_after(D.ix.search_after(*qs, k, cursors), rows, cursors, k, None, W.fields, f"ties k={k} after")


TIE_SPECS = {"const": (("const", "asc"),), "two": (("two", "asc"),), "two_score": (("two", "asc"), ("_score", "desc")),
             "const_desc_score": (("const", "desc"), ("_score", "asc"))}


@pytest.mark.parametrize("k", [1025, 2049, 3073])
@pytest.mark.parametrize("spec", list(TIE_SPECS))
def test_sorted_ties_across_ranges(dev, oracle, spec, k):
    """3 073 candidates whose field words are constant (only segment | doc vary), or take two values that change
    exactly at rank 1 024 (tie_x) and at rank 1 025 (tie_y); their scores are one bit pattern"""
    W, D = SW.ties_world(), dev("ties", "no_seed")
    names, sort = ["tie_x", "tie_y", "tie_topk"], list(TIE_SPECS[spec])
    rows = rows_of(oracle, W, "ties_sorted", names, TIE_SPECS[spec])
    cap = SW.SORTED_CAP
    assert rows[1][cap - 1].values == rows[1][cap].values   # equal field parts across the first boundary
    check_sorted_rows(D.ix.search_sorted(*W.queries(names), k, D.sort(sort)), rows, k, sort, f"{spec} k={k}")
    cursors = [None, cursor_of(rows[1][0]), None]
    got = D.ix.search_after(*W.queries(names), k, cursors, sort=D.sort(sort))
    check_after(got, rows, cursors, k, sort, W.fields, f"{spec} k={k} after")


# ---- case 4: the `all` shortcut, the final range's overshoot, the large-candidate switch --------------------
def bool_and_cursor(D, oracle, names, k, what):
    """the queries through a bool batch whose clause tables accept everything (select_topk_kernel<false> at any k)
    and through a cursor batch without cursors (<true>)"""
    W = D.W
    qs = W.queries(names)
    want = oracle.search_batch(W.segs, *qs, k, strategy=oracle.BM25)
    cl = SW.accepting_clauses(len(names), len(W.segs))
    same(D.ix.search_batch_bool(*qs, k, cl), want, f"{what} bool")
    got = D.ix.search_after(*qs, k, [None] * len(names))
    same(got[:4], want, f"{what} cursor")
    assert got[4].tolist() == [W.n[nm] for nm in names] and got[5].tolist() == [1] * len(names)


@pytest.mark.parametrize("k", SW.SMALL_KS)
def test_all_shortcut_and_overshoot(dev, oracle, k):
    """small k on the select path; n = cap_last (everything fits: no select), cap_last + 1 and 2 cap_last + 1, every
    candidate of one score: the keys taken beyond k and dropped after the sort are tied with kept ones"""
    D = dev("ties", "no_seed")
    names = [f"o{n}" for n in SW.OVERSHOOT_NS]
    assert {f"o{n}" for n in SW.overshoot_ns(k)} <= set(names)
    bool_and_cursor(D, oracle, names, k, f"overshoot k={k}")
    # a cursor inside the tie run: n - 1 - rank candidates are left
    rows = rows_of(oracle, D.W, "overshoot", names, None)
    cursors = [cursor_of(r[q % 3]) for q, r in enumerate(rows)]
    got = D.ix.search_after(*D.W.queries(names), k, cursors)
    check_after(got, rows, cursors, k, None, D.W.fields, f"overshoot k={k} cursors")


@pytest.mark.parametrize("k", SW.SWITCH_KS)
def test_large_candidate_switch(dev, oracle, k):
    """8 192 and 8 193 candidates: the two sides of n_flat > 16 * NT (cap_last = kSelectCap)"""
    bool_and_cursor(dev("ties", "no_seed"), oracle, [f"o{n}" for n in SW.SWITCH_NS], k, f"switch k={k}")


# ---- case 5: slice walking -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", SW.SLICE_KS)
def test_slice_table_and_strided_loop(dev, oracle, k):
    """queries of 1, 2, 511, 512 (the table's last size), 513 and 700 slices (the strided loop)"""
    W, D = SW.slices_world(), dev("slices", "slice")
    qs = W.queries(list(SW.SLICE_QUERIES))
    b = D.ix.prepare(*qs, k)
    try:
        assert b.info()["n_slices"] == sum(SW.SLICE_COUNTS)
    finally:
        b.close()
    want = oracle.search_batch(W.segs, *qs, k, strategy=oracle.BM25)
    same(D.ix.search_plan(*qs, k), want, f"slices k={k}")
    got = D.ix.search_after(*qs, k, [None] * len(SW.SLICE_QUERIES))
    same(got[:4], want, f"slices k={k} cursor")


def test_sorted_many_slices(dev, oracle):
    """select_sorted_kernel over 513 and 700 slices"""
    W, D = SW.slices_world(), dev("slices", "slice")
    names, sort = ["s513", "s700", "s2"], [("low", "asc"), ("_score", "desc")]
    rows = rows_of(oracle, W, "slices_sorted", names, tuple(sort))
    for k in (257, 1025):
        check_sorted_rows(D.ix.search_sorted(*W.queries(names), k, D.sort(sort)), rows, k, sort, f"slices sorted k={k}")


@pytest.mark.parametrize("k", [11, 257])
def test_empty_slices(dev, oracle, k):
    """a clustered MUST list leaves regions empty at the start, in the middle (two in a row) and at the end of the
    query's slice run, and regions of 1, 5, 64 and 128 survivors"""
    W, D = SW.slices_world(), dev("slices", "region")
    qs, cl = W.queries(["E", "E"]), SW.region_clauses(W)
    b = D.ix.prepare(*qs, k, clauses=cl)
    try:
        assert b.info()["n_slices"] == 2 * sum(len(r) for r in SW.REGION_SURVIVORS)
    finally:
        b.close()
    want = B.reference(oracle, W.segs, *qs, k, cl)
    survivors = sum(sum(r) for r in SW.REGION_SURVIVORS)
    assert want[3].tolist() == [min(k, survivors), min(k, SW.REGION * 13)]
    same(D.ix.search_batch_bool(*qs, k, cl), want, f"empty slices k={k}")
    sort = [("low", "asc"), ("_score", "desc")]
    rows = ordered_rows(B.reference(oracle, W.segs, *qs, W.k_all, cl), sort, W.fields)
    got = D.ix.search_batch_bool(*qs, k, cl, sort=D.sort(sort))
    check_sorted_rows(got[:4] + (got[-1],), rows, k, sort, f"empty slices sorted k={k}")


# ---- case 6: dropped entries inside regions ------------------------------------------------------------------
def run_twice(D, qs, k, qf, sort=None):
    """sweep 1 rewrites cand[].y in place: a second run() of the prepared batch gives the same rows"""
    b = D.ix.prepare(*qs, k, q_filter=qf, sort=D.sort(sort))
    try:
        out = []
        for _ in range(2):
            b.run()
            out.append(b.fetch() + ((b.matched_counts(),) if sort is not None else ()))
    finally:
        b.close()
    for x, y in zip(*out):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), "second run() differs"
    return out[1]


def filtered(oracle, D, names, k):
    W = D.W
    qf = SW.third_filtered(len(names), D.fid)
    qs = W.queries(names)
    return qs, qf, oracle.search_batch_filtered(W.segs, *qs, k, qf, {D.fid: D.masks}, strategy=oracle.BM25)


def test_dropped_entries_topk(dev, oracle):
    """case 1 at k = 2049 with tombstones in segment 1 and a doc filter on a third of the queries"""
    D = dev("ranges_del", "no_seed")
    qs, qf, want = filtered(oracle, D, D.W.topk_names, 2049)
    assert len(set(want[3].tolist())) > 8 and (want[3] < 2049).any() and (want[3] == 2049).any()
    same(run_twice(D, qs, 2049, qf), want, "dropped k=2049")


def test_dropped_entries_sorted(dev, oracle):
    """case 2 (four parts, k = 1025) with the same tombstones and filter"""
    D = dev("ranges_del", "no_seed")
    sort = SPECS["four_score_last"]
    qs, qf, hits = filtered(oracle, D, D.W.sorted_names, D.W.k_all)
    check_sorted_rows(run_twice(D, qs, 1025, qf, sort), ordered_rows(hits, sort, D.W.fields), 1025, sort, "dropped sorted")


def test_dropped_entries_slices(dev, oracle):
    """case 5 at k = 2049 (table and strided loop) with tombstones in segment 0 and the filter"""
    D = dev("slices_del", "slice")
    qs, qf, want = filtered(oracle, D, list(SW.SLICE_QUERIES), 2049)
    same(run_twice(D, qs, 2049, qf), want, "dropped slices k=2049")
