"""The worlds of tests/test_gpu_top_hits.py give what its cases name — checked here on the CPU with the oracle's hits
and tests/top_hits_ref.py alone, so that a GPU case that passes has met the situation it is there for."""
import numpy as np
import pytest

from tests import agg_date_ref as D
from tests import top_hits_ref as T
from tests import top_hits_world as TW


@pytest.fixture(scope="module")
def world(oracle):
    return TW.build(oracle)


def lists(W, body, rows, q=0):
    return T.lists_of(body, {"rows": rows, "first_id": 0}, W["hits"][q], W["cols"], W["masks"], TW.KEYS_OF)


def test_matched_counts_around_a_wave_and_four(world):
    n = [len(h) for h in world["hits"]]
    live = sum(int(s.docs) for s in world["segs"])
    assert 2000 < n[0] <= live < world["k_all"]  # tombstones
    assert n[10] == 0 and n[11] == 1
    assert n[9] == 40 and {s for s, _, _ in world["hits"][9]} == {0}  # fewer than a wave
    assert 64 < n[8] < 256 and {s for s, _, _ in world["hits"][8]} == {0, 1}  # fewer than four waves' worth
    assert all(64 < x for x in n[1:8])


def test_list_lengths_around_the_64_entry_read(world):
    body = {"type": "terms", "field": "len"}
    got = lists(world, body, len(TW.LEN_KEYS))
    assert [len(lst) for lst in got] == list(TW.LENGTHS) == [0, 1, 63, 64, 65, 128, 129]
    assert all(len({s for s, _, _ in lst}) == 2 for lst in got[2:])  # both segments feed every longer list
    # from at and beyond the length, for the slices the GPU cases use
    for frm, size in ((1, 1), (63, 1), (62, 1)):
        counts = [len(T.one_list(lst, size, frm, [], world["fields"])[1]) for lst in got]
        assert 0 in counts and size in counts


def test_terms_docs_with_two_keys_a_repeated_key_and_none(world):
    tag = [d for seg in world["cols"]["tag"] for d in seg]
    assert any(len(d) == 2 and d[0] != d[1] for d in tag) and any(len(d) == 2 and d[0] == d[1] for d in tag)
    assert any(len(d) == 0 for d in tag)
    body = {"type": "terms", "field": "tag", "missing": "none"}
    got = lists(world, body, len(TW.KEYS) + 1)
    n = len(world["hits"][0])
    assert len(got[-1]) > 0 and sum(map(len, got)) > n  # the missing row; docs in two lists
    twice = {(s, d) for s, seg in enumerate(world["cols"]["tag"]) for d, v in enumerate(seg) if len(v) == 2 and v[0] == v[1]}
    for lst in got:
        keys = [(s, d) for s, d, _ in lst]
        assert len(keys) == len(set(keys))  # a repeated key counts once
    assert twice & {(s, d) for s, d, _ in world["hits"][0]}


def test_overlapping_ranges_and_histograms(world):
    body = {"type": "range", "field": "x", "ranges": [{"to": 1.0}, {"from": -1.0}]}
    a, b = lists(world, body, 2)
    assert {(s, d) for s, d, _ in a} & {(s, d) for s, d, _ in b}
    for interval, rows in ((1, 9000), (2, 4500), (100, 90)):
        body = {"type": "histogram", "field": "wide", "interval": interval}
        lay = D.ref_layout([dict(body=body, parent=-1)], world["cols"], TW.KEYS_OF)[0]
        assert lay["rows"] == rows and lay["first_id"] == 0
    # 9000 rows: beyond the 8192 count cells of the aggregation kernel's LDS home and the 4096 LDS cursors
    assert 9000 * 4 > 32768 and 4500 * 4 <= 32768 and 4500 > 4096 and 90 <= 4096


def test_ties_and_missing_values(world):
    F = world["fields"]
    assert {v[0] for seg in F["tie"][0] for v in seg} == {5}
    hits = world["hits"][0]
    _, best = T.one_list(hits, 64, 0, [("tie", "asc")], F)
    assert [(s, d) for s, d, _ in best] == sorted((s, d) for s, d, _ in hits)[:64]  # segment, then doc
    missing = [h for h in hits if not F["f64"][0][h[0]][h[1]]]
    assert 64 < len(missing) < len(hits) - 64
    for order in ("asc", "desc"):
        _, best = T.one_list(hits, 64, 0, [("f64", order)], F)
        assert all(F["f64"][0][s][d] for s, d, _ in best)  # Missing after every value in both orders
    _, best = T.one_list(missing[:10], 10, 0, [("f64", "desc")], F)
    assert [(s, d) for s, d, _ in best] == sorted((s, d) for s, d, _ in missing[:10])
    low = T.one_list(hits, 64, 0, [("low", "asc"), ("_score", "desc")], F)[1]
    assert low != T.one_list(hits, 64, 0, [("low", "asc")], F)[1]  # the second part decides among the ties


def test_overflow_has_a_query_that_fits_beside_one_that_does_not(world):
    body = {"type": "terms", "field": "tag", "missing": "none"}
    need = [sum(map(len, lists(world, body, 7, q))) for q in range(12)]
    assert need[0] == max(need) and sorted(need)[-2] < need[0] - 1 and need[10] == 0


def test_many_segments_give_more_slices_than_waves(oracle):
    W = TW.build_many(oracle)
    assert len(W["segs"]) == 6 > 4
    assert len({s for s, _, _ in W["hits"][0]}) == 6  # a slice per segment at least
    assert len(W["hits"][0]) > 64
