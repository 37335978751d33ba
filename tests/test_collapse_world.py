"""The world of tests/test_gpu_collapse.py gives what its cases need — checked here on the CPU with the oracle's
rows and tests/collapse_ref.py alone, so that a GPU case that passes has met the situation it is there for."""
import numpy as np
import pytest

from tests import collapse_ref as R
from tests import collapse_world as CW


@pytest.fixture(scope="module")
def world(oracle):
    return CW.build(oracle)


def arrays(W, k, column, G, inner=None, inner_sort=None, main_sort=None):
    rows = CW.sorted_rows(W["all"], main_sort, W["fields"])
    frm, size = inner or (0, 0)
    return R.expected_arrays(*CW.as_arrays(rows, k), W["columns"][column][0], G, frm, size, inner_sort, main_sort,
                             W["fields"])


def test_row_counts_reach_every_k(world):
    n = world["all"][3]
    live = sum(int(s.docs) for s in world["segs"])
    assert world["k_all"] == 620 and live < 620  # (tombstones: no query can have 620 rows)
    assert n[14] == 0 and n[15] == 1
    for k in CW.KS[:-1]:
        assert (n >= k).any() and (n < k).any(), k  # a query is cut at k, another has fewer rows
    assert 512 < n.max() <= live  # at k = 620 every query shows all its rows: more than 512, a table of 2048 slots


def test_groups_above_and_below_the_limit_and_dropped_rows(world):
    for k in (65, 620):
        a = arrays(world, k, "seven", 3)
        assert (a["total_groups"] > 3).any() and (a["total_groups"] < 3).any()
        assert (a["group_size"].sum(axis=1) < np.minimum(world["all"][3], k)).any()  # rows without a value
    a = arrays(world, 620, "noseg", 7)
    seg1 = [sum(1 for s, _, _ in rows if s == 1) for rows in CW.sorted_rows(world["all"], None, world["fields"])]
    assert max(seg1) > 50  # every row of segment 1 is dropped
    assert a["group_size"][0].sum() <= world["all"][3][0] - seg1[0]


def test_one_group_holds_more_members_than_a_wave(world):
    a = arrays(world, 620, "one", 1, (0, 64), [("low", "asc")])
    assert a["group_size"][0, 0] > 2 * 64 + 1 and a["inner_count"][0, 0] == 64
    b = arrays(world, 620, "one", 1, (0, 64))
    assert not np.array_equal(a["inner_row"], b["inner_row"])  # the inner sort moves them
    assert np.array_equal(b["inner_row"][0, 0], np.arange(1, 65))
    c = arrays(world, 620, "one", 1, (600, 1))
    assert not c["inner_count"].any()  # from >= members everywhere


def test_inner_sort_ties_differ_from_row_order(world):
    a = arrays(world, 257, "seven", 7, (0, 64), [("low", "asc")])
    rows = a["inner_row"][0, 0, :a["inner_count"][0, 0]].tolist()
    assert len(rows) > 8 and rows != sorted(rows)
    low = world["fields"]["low"][0]
    keys = [(low[s][d][0], s, d) for s, d in zip(a["inner_seg"][0, 0, :len(rows)].tolist(),
                                                a["inner_doc"][0, 0, :len(rows)].tolist())]
    assert keys == sorted(keys) and len({k[0] for k in keys}) < len(keys)  # ties, broken by (segment, doc)


def test_own_ordinals_and_probe_chains(world):
    a = arrays(world, 620, "own", 620)
    assert np.array_equal(a["total_groups"], world["all"][3]) and (a["group_size"][0, :a["n_groups"][0]] == 1).all()
    big = world["columns"]["big"][0]
    ords = {v[0] for col in big for v in col}
    assert all(o % 8192 in (0, 1) for o in ords) and max(ords) < CW.BIG_ORDS and len(ords) > 100


def test_multi_valued_rows_fail_some_queries_only(world):
    for k in (64, 620):
        st = arrays(world, k, "multi", 5)["status"]
        assert st.any() and not st.all(), k
    assert arrays(world, 1, "multi", 1)["status"].sum() <= 1
