"""tests/collapse_ref.py against tables whose expected output is derived by hand from api/reader.rs:3499-3562
(collapse_hits) and :3578-3595 (collapse_value), and properties of it on random rows.  CPU only."""
import numpy as np
import pytest

from tests import collapse_ref as R

# one segment of 10 docs, ordinals by doc:   doc  0    1    2    3    4     5    6    7    8    9
COL = [[[2], [5], [2], [], [5], [2], [7], [], [2], [5]]]
# rows in main order (score desc): (seg, doc, score)
ROWS = [(0, 3, 9.0), (0, 0, 8.0), (0, 1, 7.0), (0, 2, 6.0), (0, 7, 5.5), (0, 4, 5.0), (0, 6, 4.0), (0, 5, 3.0),
        (0, 8, 2.0), (0, 9, 1.0)]


def groups(rows=ROWS, col=COL, **kw):
    return [(top, o, members) for top, o, members, _ in R.collapse_hits(rows, col, **kw)]


def test_first_appearance_order_and_a_dropped_first_row():
    """row 0 (doc 3) has no value: it is dropped, not a group of its own and nobody's member (:3508-3510); the
    groups come in the order their first row appears (:3511-3513): ordinal 2 (row 1), 5 (row 2), 7 (row 6)"""
    got = R.collapse_hits(ROWS, COL, inner={"size": None, "sort": None})
    assert [(top, o) for top, o, _, _ in got] == [(1, 2), (2, 5), (6, 7)]
    assert [m for _, _, m, _ in got] == [[3, 7, 8], [5, 9], []]  # the representative is never its own member
    assert [size for *_, size in got] == [4, 3, 1]
    # rows 0 and 4 (docs 3 and 7, no value) appear nowhere
    assert not {0, 4} & {i for top, _, m, _ in got for i in [top] + m}


def test_without_inner_hits_members_are_discarded():
    assert groups() == [(1, 2, []), (2, 5, []), (6, 7, [])]  # (:3554-3556)


def test_a_multi_valued_row_fails_the_query():
    col = [[list(v) for v in COL[0]]]
    col[0][6] = [7, 2]  # doc 6, row 6
    with pytest.raises(R.MultiValued):
        R.collapse_hits(ROWS, col)
    # a multi-valued doc that is not among the rows does not matter
    assert groups(ROWS[:6], col) == [(1, 2, []), (2, 5, [])]


def test_from_and_size():
    g = lambda frm, size: [m for _, _, m in groups(inner={"from": frm, "size": size, "sort": None})]
    assert g(0, 1) == [[3], [5], []]
    assert g(1, 2) == [[7, 8], [9], []]
    assert g(2, 5) == [[8], [], []]  # from == members of the second group: cleared (:3541-3542)
    assert g(3, 1) == [[], [], []]   # from >= members everywhere
    assert g(0, 0) == [[], [], []]   # size 0 keeps none (:3548-3549)
    assert g(0, None) == [[3, 7, 8], [5, 9], []]


def test_inner_sort_ties_fall_to_segment_and_doc_not_to_the_main_order():
    """two segments; the members of ordinal 1 tie on the inner field and must come out by (segment, doc) — the
    full SortKey of resort_hits (:3564-3576) — which is not their main (score) order"""
    col = [[[1], [1], [1]], [[1], [1]]]
    fields = {"f": ([[[4], [4], [3]], [[4], [4]]], False)}
    rows = [(1, 1, 9.0), (0, 1, 8.0), (1, 0, 7.0), (0, 2, 6.0), (0, 0, 5.0)]
    got = groups(rows, col, inner={"size": None, "sort": [("f", "asc")]}, fields=fields)
    # representative: row 0; members by f asc: row 3 (f = 3), then f = 4 by (seg, doc): (0,0) row 4, (0,1) row 1, (1,0) row 2
    assert got == [(0, 1, [3, 4, 1, 2])]
    # under the main order they would be rows 1, 2, 3, 4
    assert groups(rows, col, inner={"size": None, "sort": None}) == [(0, 1, [1, 2, 3, 4])]
    # from / size apply after the re-sort (:3540-3553)
    assert groups(rows, col, inner={"from": 1, "size": 2, "sort": [("f", "asc")]}, fields=fields) == [(0, 1, [4, 1])]


def test_an_empty_inner_sort_is_score_desc():
    """query/sort.rs:159-167; against a field-sorted request it differs from the main order, and with the
    MatchOnly scores 0.0 of such a request every member ties: (segment, doc) order"""
    col = [[[1]] * 4]
    fields = {"f": ([[[1], [2], [3], [4]]], False)}
    rows = [(0, 3, 0.0), (0, 2, 0.0), (0, 1, 0.0), (0, 0, 0.0)]  # main order: f desc
    same = dict(rows=rows, col=col, main_sort=[("f", "desc")], fields=fields)
    assert groups(inner={"size": None, "sort": []}, **same) == [(0, 1, [3, 2, 1])]
    assert groups(inner={"size": None, "sort": None}, **same) == [(0, 1, [1, 2, 3])]
    # in score order an empty inner sort IS the main order: no re-sort, whatever the scores' ties would do
    rows2 = [(0, 2, 5.0), (0, 3, 5.0), (0, 0, 1.0), (0, 1, 1.0)]
    assert groups(rows2, col, inner={"size": None, "sort": []}) == [(0, 1, [1, 2, 3])]
    # with scores, `_score` asc reverses the members but not the representative
    assert groups(rows2, col, inner={"size": None, "sort": [("_score", "asc")]}) == [(0, 1, [2, 3, 1])]


def test_expected_arrays_layout():
    doc = np.array([[r[1] for r in ROWS]], np.uint32)
    seg = np.zeros_like(doc)
    score = np.array([[r[2] for r in ROWS]], np.float32)
    a = R.expected_arrays(doc, seg, score, np.array([10], np.uint32), COL, group_limit=2, inner_from=1, inner_size=2)
    assert a["total_groups"].tolist() == [3] and a["n_groups"].tolist() == [2] and a["status"].tolist() == [0]
    assert a["group_row"].tolist() == [[1, 2]] and a["group_ord"].tolist() == [[2, 5]]
    assert a["group_size"].tolist() == [[4, 3]] and a["group_doc"].tolist() == [[0, 1]]
    assert a["group_score"].tolist() == [[8.0, 7.0]] and a["inner_count"].tolist() == [[2, 1]]
    assert a["inner_row"].tolist() == [[[7, 8], [9, 0]]] and a["inner_doc"].tolist() == [[[5, 8], [9, 0]]]
    col = [[list(v) for v in COL[0]]]
    col[0][9] = [5, 5]
    b = R.expected_arrays(doc, seg, score, np.array([10], np.uint32), col, group_limit=2, inner_size=2)
    assert b["status"].tolist() == [1] and not any(v.any() for n, v in b.items() if n != "status")
    c = R.expected_arrays(doc, seg, score, np.array([9], np.uint32), col, group_limit=2)  # the row is not reached
    assert c["status"].tolist() == [0] and c["group_size"].tolist() == [[4, 2]]
    assert c["inner_row"].shape == (1, 2, 0)


def random_world(seed):
    rng = np.random.default_rng(seed)
    n_docs = [40, 25]
    col = [[[] if rng.random() < 0.15 else [int(rng.integers(0, 6))] for _ in range(n)] for n in n_docs]
    fields = {"f": ([[[int(rng.integers(0, 4))] for _ in range(n)] for n in n_docs], False)}
    rows = [(s, d, float(np.float32(rng.integers(0, 5)))) for s, n in enumerate(n_docs) for d in range(n)]
    rows = [rows[i] for i in rng.permutation(len(rows))[:int(rng.integers(0, len(rows) + 1))]]
    rows.sort(key=R.sort_key(R.SCORE_DESC, fields))
    return rows, col, fields


@pytest.mark.parametrize("seed", range(12))
def test_properties_on_random_rows(seed):
    rows, col, fields = random_world(seed)
    valued = [i for i, (s, d, _) in enumerate(rows) if col[s][d]]
    everything = {"from": 0, "size": len(rows) + 1}
    got = R.collapse_hits(rows, col, inner=dict(everything, sort=[("f", "asc")]), fields=fields)
    tops = [top for top, *_ in got]
    assert tops == sorted(tops)  # representatives are a subsequence of the rows
    for top, o, members, size in got:
        s, d, _ = rows[top]
        assert col[s][d] == [o]
        assert top == min(i for i in valued if col[rows[i][0]][rows[i][1]] == [o])  # the first row of its ordinal
        assert size == 1 + len(members) and top not in members
    # representatives plus members partition the rows that have a value
    assert sorted(tops + [i for _, _, m, _ in got for i in m]) == valued
    # an inner sort given explicitly and equal to the request's own gives what none gives
    plain = R.collapse_hits(rows, col, inner=dict(everything, sort=None))
    assert R.collapse_hits(rows, col, inner=dict(everything, sort=[("_score", "desc")])) == plain
    assert R.collapse_hits(rows, col, inner=dict(everything, sort=[])) == plain
    by_f = sorted(rows, key=R.sort_key([("f", "asc")], fields))
    plain_f = R.collapse_hits(by_f, col, inner=dict(everything, sort=None), main_sort=[("f", "asc")], fields=fields)
    assert R.collapse_hits(by_f, col, inner=dict(everything, sort=[("f", "asc")]), main_sort=[("f", "asc")],
                           fields=fields) == plain_f
    for _, _, members, _ in plain_f:
        assert members == sorted(members)  # the main order is the row order
