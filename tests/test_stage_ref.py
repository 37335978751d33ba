"""tests/stage_ref.py pinned on the CPU: the oracle's impacts against the numpy restatement on the whole value grid
of tests/stage_worlds.py, the reference facts that grid relies on, and the champion checker against hand-made
tables it has to refuse."""
import numpy as np
import pytest

from tests import stage_ref as R
from tests import stage_worlds as SW

F32 = np.float32
bits = lambda a: np.asarray(a, dtype=F32).view(np.uint32)


def ulp(x, n=1):
    """x moved by n ulps (a positive finite f32, or 0)"""
    return (np.array([x], dtype=F32).view(np.int32) + np.int32(n)).view(F32)[0]


@pytest.mark.parametrize("si", range(len(SW.V_PARAMS)))
def test_oracle_and_numpy_impacts_agree_on_the_value_grid(oracle, si):
    seg = SW.v_segments()[si]
    assert np.array_equal(bits(R.impacts(oracle, seg)), bits(R.impacts_np(seg)))
    for deleted, live in SW.v_updates():  # the re-derivation's `docs`
        s = SW.with_update(seg, deleted, live)
        assert np.array_equal(bits(R.impacts(oracle, s)), bits(R.impacts_np(s))), live


def test_oracle_and_numpy_impacts_agree_on_the_champion_world(oracle):
    seg = SW.c_segment()
    assert np.array_equal(bits(R.impacts(oracle, seg)), bits(R.impacts_np(seg)))


def test_reference_facts_the_grid_relies_on(oracle):
    assert oracle.bm25(1.0, 1.0, 0.0, 0.0, 10.0, 1.2, 0.75) > 0  # query/bm25.rs's own test: avgdl 0
    # docs < df: the logarithm's argument is negative, max(0.0) drops the NaN, idf = 1
    for docs, df in ((202.0, 203.0), (1.0, 68.0), (40.0, 68.0), (1.0, 2.0)):
        assert R.idf_np(docs, df) == F32(1.0)
        with_idf = oracle.bm25(2.0, df, 5.0, 5.0, docs, 1.2, 0.75)
        assert bits(with_idf) == bits(F32(F32(2.0) * F32(F32(1.2) + F32(1.0))) / F32(F32(2.0) + F32(F32(1.2) * F32(F32(F32(1.0) - F32(0.75)) + F32(0.75)))))
    # a missing length under avgdl = 0.25 counts as max(avgdl, 1) = 1.0, not as 0.25
    seg = SW.v_segments()[0]
    lens1 = seg.field_doc_len[1]
    missing = int(np.nonzero(lens1 == 0)[0][0])
    assert R.doc_len(seg, 1, missing) == 1.0 and seg.field_avgdl[1] == F32(0.25)
    assert R.doc_len(seg, 0, 1) == 7.5 and seg.field_doc_len[0][1] == F32(-3.0)  # a negative length is missing too
    assert R.doc_len(seg, 2, 0) == 3.0 and seg.field_doc_len[2] is None
    assert R.doc_len(seg, 3, 0) == 1.0 and seg.field_avgdl[3] == 0
    assert oracle.score_tf(1.0, 1.0, 1.0, 0.25, 10.0, 1.2, 0.75, 1.0) != oracle.score_tf(1.0, 1.0, 0.25, 0.25, 10.0, 1.2, 0.75, 1.0)


# ---- the champion checker ---------------------------------------------------------------------------------
def small_world():
    """lists of 3, 70 and 300 postings with distinct positive impacts, and one of 200 equal ones"""
    from searchlite_amd.segment import Segment
    dfs = (3, 70, 300, 200)
    n = 300
    offs = np.concatenate([[0], np.cumsum(dfs)]).astype(np.uint64)
    docs = np.concatenate([np.arange(d) for d in dfs]).astype(np.uint32)
    tfs = np.concatenate([1 + (np.arange(d) * 11) % d if i < 3 else np.ones(d, dtype=np.int64) for i, d in enumerate(dfs)]).astype(np.uint32)
    return Segment(n_docs=n, term_offsets=offs, doc_ids=docs, tfs=tfs, field_doc_len=[np.full(n, 900.0, dtype=F32)],
                   field_avgdl=np.array([3.0], dtype=F32), docs=float(n), k1=1.2, b=0.75)


def good_table(seg, imps):
    dead = R.deleted_mask(seg)
    rows = []
    for t in range(seg.n_terms):
        a, b = int(seg.term_offsets[t]), int(seg.term_offsets[t + 1])
        rows.append(R.lane_table(np.where(dead[seg.doc_ids[a:b]], F32(0.0), imps[a:b])))
    return np.stack(rows)


def test_checker_accepts_valid_tables_and_lower_bounds(oracle):
    seg = small_world()
    imps = R.impacts(oracle, seg)
    for t in range(3):
        x = imps[int(seg.term_offsets[t]):int(seg.term_offsets[t + 1])]
        assert len(np.unique(x)) == len(x) and (x > 0).all()
    tab = good_table(seg, imps)
    R.check_champions(tab, seg, imps)
    low = tab.copy()
    low[2, 5] = ulp(low[2, 6], 1) if low[2, 6] < low[2, 5] else low[2, 5]  # a rank bound that is low but positive
    low[2, 64] = ulp(low[2, 64], -3)
    R.check_champions(low, seg, imps)
    dead = np.zeros(seg.n_docs, dtype=bool)
    dead[[0, 1, 64, 128, 299]] = True
    s2 = SW.with_update(seg, np.packbits(dead, bitorder="little"), float(seg.n_docs - dead.sum()))
    imps2 = R.impacts(oracle, s2)
    R.check_champions(good_table(s2, imps2), s2, imps2)
    with pytest.raises(AssertionError):
        R.check_champions(good_table(seg, imps2), s2, imps2)  # a table that counts the dead postings


@pytest.mark.parametrize("what", ["max one ulp low", "max one ulp high", "rank bound one ulp high", "rank 128 bound one ulp high",
                                  "positive past a short list", "positive rank 512 bound of 300 postings",
                                  "zero where a bound is due", "zero rank 256 bound of 300 postings", "increasing",
                                  "equal list with another value"])
def test_checker_refuses(oracle, what):
    seg = small_world()
    imps = R.impacts(oracle, seg)
    tab = good_table(seg, imps)
    R.check_champions(tab, seg, imps)
    if what == "max one ulp low":
        tab[1, 0] = ulp(tab[1, 0], -1)
    elif what == "max one ulp high":
        tab[1, 0] = ulp(tab[1, 0], 1)
    elif what == "rank bound one ulp high":
        desc = np.sort(imps[int(seg.term_offsets[2]):int(seg.term_offsets[3])])[::-1]
        tab[2, 9] = ulp(desc[9], 1)  # (still below row[8]: only the order statistic refuses it)
        assert tab[2, 9] < tab[2, 8]
    elif what == "rank 128 bound one ulp high":
        desc = np.sort(imps[int(seg.term_offsets[2]):int(seg.term_offsets[3])])[::-1]
        tab[2, 64] = ulp(desc[127], 1)
    elif what == "positive past a short list":
        tab[0, 3] = tab[0, 2]
    elif what == "positive rank 512 bound of 300 postings":
        tab[2, 66] = ulp(F32(0.0), 1)
    elif what == "zero where a bound is due":
        tab[1, 63] = 0.0
    elif what == "zero rank 256 bound of 300 postings":
        tab[2, 65] = 0.0  # (300 >= 256: each of the 64 lanes holds 4 postings)
    elif what == "increasing":
        tab[2, 10], tab[2, 11] = tab[2, 11], tab[2, 10]
        assert tab[2, 10] < tab[2, 11]
    else:
        tab[3, 64] = ulp(tab[3, 64], -1)
    with pytest.raises(AssertionError):
        R.check_champions(tab, seg, imps)


# ---- filters ----------------------------------------------------------------------------------------------
def test_filter_pass_on_known_values():
    from searchlite_amd.segment import Segment
    seg = Segment(n_docs=5, term_offsets=[0, 2, 3], doc_ids=[0, 4, 2], tfs=[1, 1, 1], field_doc_len=[np.ones(5)],
                  field_avgdl=[1.0], docs=4.0, deleted=np.packbits([0, 1, 0, 0, 0], bitorder="little"))
    t, f = True, False
    assert R.filter_pass("bitmap", None, seg).tolist() == [t, f, t, t, t]
    assert R.filter_pass("bitmap", [t, t, f, f, f], seg).tolist() == [t, f, f, f, f]
    col = np.array([SW.P53, SW.P53 + 1, SW.P53 + 1, SW.I64_MIN, SW.I64_MAX], dtype=np.int64)
    assert R.filter_pass("i64", (col, SW.P53, SW.P53), seg).tolist() == [t, f, f, f, f]  # (double would pass 2^53 + 1)
    assert R.filter_pass("i64", (col, SW.I64_MIN, SW.I64_MAX), seg).tolist() == [t, f, t, t, t]
    fc = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf])
    assert R.filter_pass("f64", (fc, -np.inf, np.inf), seg).tolist() == [f, f, t, t, t]
    assert R.filter_pass("f64", (fc, 0.0, -0.0), seg).tolist() == [f, f, t, f, f]
    assert R.filter_pass("terms", ([0, SW.NO_TERM], True, None), seg).tolist() == [f, f, t, t, f]
    assert R.filter_pass("terms", ([0, 1], False, [t, t, t, t, f]), seg).tolist() == [t, f, t, f, f]
    assert R.filter_pass("terms", ([], True, None), seg).tolist() == [t, f, t, t, t]
    assert not R.filter_pass("terms", ([], False, None), seg).any()
