"""The worlds of tests/test_gpu_stage_edges.py hold every edge their cases are there for — asserted on the CPU, on
the worlds and the reference alone, so that a GPU case that passes has met the situation it is named after."""
import numpy as np
import pytest

from tests import stage_ref as R
from tests import stage_worlds as SW

F32 = np.float32
TINY = np.finfo(np.float32).tiny  # the smallest normal f32


def lists_of(seg):
    return [seg.postings(t) for t in range(seg.n_terms)]


# ---- V -------------------------------------------------------------------------------------------------------
def test_v_layout_lists_fields_and_tfs():
    offs, docs, tfs, tfield, names = SW.v_layout()
    df = np.diff(offs.astype(np.int64))
    assert df[0] == 0 and df[-1] == 0 and 0 in df[1:-1]  # empty lists: first, middle, last term
    assert 1 in df and SW.V_DOCS in df and 150 < SW.V_DOCS < 256
    assert sorted(set(tfield.tolist())) == [0, 1, 2, 3, 4]
    term = np.repeat(np.arange(len(df)), df)
    for f in range(5):  # every field meets every tf value, in a list of every doc
        full = [t for t in range(len(df)) if tfield[t] == f and df[t] == SW.V_DOCS]
        assert full
        assert set(tfs[term == full[0]].tolist()) == set(SW.V_TFS)
    assert {0, 1, 2, 2 ** 24, 2 ** 24 + 1, 2 ** 32 - 1} <= set(SW.V_TFS)
    assert F32(np.uint32(2 ** 24 + 1)) == F32(2 ** 24) and F32(np.uint32(2 ** 32 - 1)) == F32(2 ** 32)  # what f32 makes of them
    # every length value of field 0 meets every tf value in the field's full list
    l0 = SW.v_lengths()[0]
    t0 = [t for t in range(len(df)) if tfield[t] == 0 and df[t] == SW.V_DOCS][0]
    pairs = {(float(l0[d]), int(x)) for d, x in zip(docs[term == t0], tfs[term == t0])}
    assert len(pairs) == len(set(np.array(SW.V_LENS0, dtype=F32).tolist())) * len(SW.V_TFS)
    for s in SW.v_segments():  # a valid descriptor: ids strictly increasing within a list and below n_docs
        for d, _ in lists_of(s):
            assert (np.diff(d.astype(np.int64)) > 0).all() and (d < s.n_docs).all()


def test_v_lengths_averages_and_parameters():
    segs = SW.v_segments()
    assert [(s.k1, s.b) for s in segs] == [(0.9, 0.4), (0.0, 0.75), (1.2, 0.0), (1.2, 1.0), (2.0, 0.75)]
    l0, l1, l2, l3, l4 = segs[0].field_doc_len
    avg = segs[0].field_avgdl
    assert avg.tolist() == [7.5, 0.25, 3.0, 0.0, F32(1e30)]
    assert {0.0, -3.0, 0.5, 1.0, float(F32(1e30)), float(F32(3e38))} <= set(l0.tolist()) and (l0 == 7.0).any()
    assert (l1 == 0).mean() > 0.6 and (l1 == 0.25).any() and (l1 > 1e37).any()
    assert l2 is None and l3 is not None and (l4 == 0).any() and (l4 > 1e38).any()
    docs = [s.docs for s in segs]
    assert docs.count(float(SW.V_DOCS)) == 2 and docs.count(float(SW.V_FULL_DF - 1)) == 2 and docs.count(1.0) == 1
    for s in segs:  # docs < df somewhere in every segment but the ones with docs = n_docs
        df = np.diff(s.term_offsets.astype(np.int64))
        assert (df > s.docs).any() == (s.docs < SW.V_DOCS)


def test_v_impacts_are_finite_and_one_is_denormal(oracle):
    denormal = 0
    for s in SW.v_segments():
        for deleted, live in [(None, s.docs)] + SW.v_updates():
            imps = R.impacts(oracle, SW.with_update(s, deleted, live))
            assert np.isfinite(imps).all() and (imps >= 0).all()
            denormal += int(((imps > 0) & (imps < TINY)).sum())
            assert (imps == 0).any()  # tf 0
    assert denormal > 0


def test_v_updates_and_queries():
    ups = SW.v_updates()
    bm = [np.unpackbits(u[0], bitorder="little")[:SW.V_DOCS].astype(bool) for u in ups[:2]]
    assert bm[0][0] and bm[0][-1] and (bm[1] >= bm[0]).all() and bm[1].sum() > bm[0].sum()  # they grow
    offs = SW.v_layout()[0]
    df = np.diff(offs.astype(np.int64))
    assert ((df > ups[1][1]) & (df < SW.V_DOCS)).any()  # docs below a df that is not the full one
    assert ups[2][0] is None and ups[2][1] not in (ups[0][1], ups[1][1], float(SW.V_DOCS))
    for n in (1, 3, 7):
        qo, qt, w = SW.v_queries(n)
        assert (np.diff(qo) == n).all() and qt.shape == (qo[-1], 5) and (w == 1).all()
    one = SW.v_queries(1)[1][:, 0]
    assert sorted(one.tolist()) == [t for t in range(len(df)) if df[t] > 0]
    assert set(SW.v_queries(3)[1][:, 0].tolist()) >= {t for t in range(len(df)) if df[t] == 0}  # empty lists in queries


# ---- C -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cworld(oracle):
    seg = SW.c_segment()
    return seg, R.impacts(oracle, seg)


def test_c_list_lengths_and_layouts(cworld):
    seg, imps = cworld
    assert {0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049} <= set(SW.C_DFS)
    assert seg.n_terms == len(SW.C_DFS) * 4 and (imps[seg.tfs > 0] > 0).all() and (seg.tfs > 0).all()
    for df in SW.C_DFS:
        for layout in SW.C_LAYOUTS:
            t = SW.c_term(df, layout)
            d, _ = seg.postings(t)
            x = imps[int(seg.term_offsets[t]):int(seg.term_offsets[t + 1])]
            assert len(d) == df and (np.diff(d.astype(np.int64)) > 0).all()
            if layout == "equal":
                assert len(np.unique(x)) == min(df, 1)
                continue
            assert len(np.unique(x)) == df  # distinct
            if layout == "desc":
                assert (np.diff(x) < 0).all()
            elif layout == "asc":
                assert (np.diff(x) > 0).all()
            else:  # the largest min(64, lane's share) impacts sit in one lane, so one lane's top 16 cannot hold them
                top = np.argsort(-x, kind="stable")[:min(64, len(x[SW.C_LANE::64]))]
                assert (top % 64 == SW.C_LANE).all()
    top = np.argsort(-imps[int(seg.term_offsets[SW.c_term(4160, "lane")]):][:4160], kind="stable")[:64]
    assert (top % 64 == SW.C_LANE).all() and len(top) == 64  # the 64 largest in one lane


def test_c_tombstones(cworld):
    seg, imps = cworld
    bm, live = SW.c_tombstones(seg)
    dead = np.unpackbits(bm, bitorder="little")[:seg.n_docs].astype(bool)
    assert dead[0] and dead[-1] and live == seg.n_docs - dead.sum()
    t = SW.c_term(2049, "desc")
    d, _ = seg.postings(t)
    assert dead[d[:30]].all() and not dead[d[30]]  # the 30 largest impacts of a descending list
    d, _ = seg.postings(SW.c_term(1025, "asc"))
    lanes = np.arange(len(d)) % 64
    assert any(dead[d[lanes == l]].all() for l in range(64))  # a whole lane's postings
    assert set(SW.C_KS) == {1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024}
    for n in (1, 3):
        qo, qt, _ = SW.c_queries(n)
        assert (np.diff(qo) == n).all() and qt.max() < seg.n_terms
    assert {SW.c_term(df, "equal") for df in SW.C_DFS if df} <= set(SW.c_queries(1)[1][:, 0].tolist())


# ---- F -------------------------------------------------------------------------------------------------------
def test_f_segments_columns_and_terms():
    W = SW.f_world()
    segs = W["segs"]
    assert [s.n_docs for s in segs] == [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000]
    last_dead = [bool(R.deleted_mask(s)[-1]) for s in segs]
    assert any(last_dead) and not all(last_dead)
    big = np.concatenate(W["i64"])
    assert {SW.I64_MIN, SW.I64_MAX, SW.P53 + 1, -(SW.P53 + 1), 0, SW.P53} <= set(big.tolist())
    assert float(np.int64(SW.P53 + 1)) == float(SW.P53)  # a conversion to double moves it onto the bound
    f = np.concatenate(W["f64"])
    assert np.isnan(f).any() and np.isposinf(f).any() and np.isneginf(f).any()
    assert (np.signbit(f) & (f == 0)).any() and (~np.signbit(f) & (f == 0)).any()
    for bound in (SW.F64_LO, SW.F64_HI):
        assert {np.nextafter(bound, -np.inf), bound, np.nextafter(bound, np.inf)} <= set(f[~np.isnan(f)].tolist())
    for s in (9, 10):  # every value of both columns in the segments large enough
        assert len(set(W["i64"][s].tolist())) == len(SW.I64_VALUES)
    T = W["terms"]
    dfs = {segs[s].df(int(T[j, s])) for j in range(4) for s in range(len(segs)) if T[j, s] != SW.NO_TERM}
    assert dfs == {1, 255, 256, 257}
    for j in range(4):
        assert (T[j] == SW.NO_TERM).any() and (T[j] != SW.NO_TERM).any()  # absent from some segments
    for s, seg in enumerate(segs):
        assert set(seg.postings(int(T[4, s]))[0].tolist()) == {0, seg.n_docs - 1}
        for d, _ in lists_of(seg):
            assert (np.diff(d.astype(np.int64)) > 0).all() and (d < seg.n_docs).all()


def test_f_cases_hit_their_edges():
    W = SW.f_world()
    cases = {name: (kind, args) for name, kind, args in SW.f_cases(W)}
    big = len(W["segs"]) - 1
    passing = lambda name, s=big: R.filter_pass(cases[name][0], cases[name][1][s], W["segs"][s])
    col = W["i64"][big]
    assert passing("i64 2^53 alone").sum() == (col == SW.P53).sum() > 0
    assert (col.astype(np.float64) == float(SW.P53)).sum() > (col == SW.P53).sum()  # a compare in double passes more
    assert not passing("i64 lo > hi").any() and not passing("f64 lo > hi").any()
    assert passing("i64 full").sum() == (~R.deleted_mask(W["segs"][big])).sum()
    assert passing("i64 hi on a value")[col == SW.P53 + 1].any()  # `<` for `<=` on the upper bound would lose these
    assert passing("i64 lo on a value")[col == -(SW.P53 + 1)].any()
    assert passing("i64 hi = max")[col == SW.I64_MAX].any() and passing("i64 lo = min")[col == SW.I64_MIN].any()
    f = W["f64"][big]
    live = ~R.deleted_mask(W["segs"][big])
    assert np.array_equal(passing("f64 (-inf, inf)"), ~np.isnan(f) & live) and np.isnan(f).any()
    assert np.array_equal(passing("f64 [inf, inf]"), np.isposinf(f) & live)
    assert np.array_equal(passing("f64 [-0.0, 0.0]"), (f == 0) & live) and passing("f64 [-0.0, 0.0]").sum() > 1
    on, inside, outside = (passing("f64 " + n).sum() for n in ("on the values", "one ulp inside", "one ulp outside"))
    assert inside < on < outside  # the neighbours of both bounds are in the column
    assert passing("bitmap first").sum() == 1 and passing("bitmap last").sum() == 0  # (the last doc of 1000 is dead)
    assert passing("bitmap last", 0).sum() == 1 and not passing("bitmap empty").any()
    for tag in ("absent", "present"):
        for j in range(5):
            a = passing(f"terms {tag} term {j}")
            assert a.any() and not a[live].all()
        assert passing(f"terms {tag} no term").all() == (tag == "absent") or not live.all()
        assert cases[f"terms {tag} and_masks"][1][2][2] is None and cases[f"terms {tag} and_masks"][1][3][2] is not None
    assert np.array_equal(passing("terms absent term 1") | passing("terms present term 1"), live)
    ups = SW.f_updates(W)
    assert len(ups) == 2
    for s, (bm, ld) in ups.items():
        old, new = R.deleted_mask(W["segs"][s]), np.unpackbits(bm, bitorder="little")[:W["segs"][s].n_docs].astype(bool)
        assert (new >= old).all() and new.sum() > old.sum() and ld == len(new) - new.sum() and new[0]


# ---- B -------------------------------------------------------------------------------------------------------
def test_b_has_more_postings_than_the_staging_grid_has_threads():
    seg = SW.b_segment()
    assert seg.n_postings > SW.B_GRID == 256 * 32 * 256 and seg.n_postings - SW.B_GRID > seg.n_docs  # the last list too
    assert seg.n_docs == 70_000 and seg.n_terms == 31 and (np.diff(seg.term_offsets.astype(np.int64)) == 70_000).all()
    assert np.array_equal(seg.postings(30)[0], np.arange(70_000))
    bm, live = SW.b_tombstones()
    dead = np.unpackbits(bm, bitorder="little")[:seg.n_docs].astype(bool)
    assert dead[0] and dead[-1] and live == seg.n_docs - dead.sum()
