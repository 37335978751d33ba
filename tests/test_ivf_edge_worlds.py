"""The worlds of tests/ivf_edge_worlds.py reach the edges they are named after.  Runs without a device: the list
lengths, the mirror's chunk, slot, pass, step and range counts, the item counts and the "straddles" conditions of every
world, and the exactness of the reference's scores.  tests/test_gpu_vector_ivf_edges.py compares the device with the
same worlds; these assertions are what makes its passing mean something."""
import numpy as np
import pytest

from tests import ivf_edge_worlds as W

METRICS = [0, 1]


def filtered(w, case):
    return W.reference(w, case, "filtered")


def flat_lens(w):
    return np.concatenate([l.lens for l in W.world_lists(w) if l is not None])


# ---- the reference's scores are exact: two orders of f32 additions give the f64 value's bytes ----
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", W.SEARCH_WORLDS)
def test_scores_are_exact_in_f32(name, metric):
    w = W.world(name, metric)
    rng = np.random.default_rng(1)
    assert w.dim <= 64 and set(np.unique(w.boost)) <= {-1.0, 0.5, 1.0}
    for s in w.segs:
        for a in (s.vals, s.cents, w.qv):
            if a is not None:
                assert np.abs(a).max() <= 1.0 and np.array_equal(a * 16, np.round(a * 16))
        W.check_exact(w.metric, w.qv, s.vals, rng, 10)
        if s.cents is not None:
            W.check_exact(w.metric, s.vals, s.cents, rng, 10)
            W.check_exact(w.metric, w.qv, s.cents, rng, 10)


# ---- A: list chunks ----
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", sorted(W.A_LENGTHS))
def test_a_worlds_reach_the_chunk_edges(name, metric):
    w = W.world(name, metric)
    lens = W.world_lists(w)[0].lens
    assert lens.tolist() == W.A_LENGTHS[name]
    nq = len(w.qv)
    for case in w.cases:
        nprobe, cand, _ = case
        pl = W.plan(w, nq, nprobe, cand)
        assert (pl.list_chunks, pl.list_chunk_docs) == W.A_CHUNKS[name]
        assert pl.list_chunk_docs % 128 == 0 and pl.list_chunk_docs * pl.list_chunks >= pl.max_len
        assert pl.slots_q == pl.P * pl.list_chunks
        ref = filtered(w, case)
        c = np.bincount(ref.probes.ravel(), minlength=len(lens))
        assert c[0] >= 129   # the longest list: three query tiles x all its chunks
        assert W.count_items(w, ref, pl, nq) >= 3 * pl.list_chunks
        # a list shorter than a chunk is probed: its later slots stay at the memset's zeros
        assert any(c[l] and 0 < lens[l] <= pl.list_chunk_docs for l in range(len(lens)))
        if nprobe >= 2 and 0 in W.A_LENGTHS[name]:
            assert c[W.A_LENGTHS[name].index(0)] > 0   # ... and so is the empty list
        if cand >= 32:
            for variant in ("filtered", "boost"):
                r = W.reference(w, case, variant)
                straddles = 0
                for q in range(nq):
                    chunks = {}
                    for f in r.top[q]:
                        s, l, ch = W.chunk_of(w, pl, f)
                        chunks.setdefault(l, set()).add(ch)
                    straddles += any(len(v) >= 2 for v in chunks.values())
                assert straddles >= 1, f"{name} {case} {variant}: no top list holds two chunks of one list"
    # every number of chunks 1 .. list_chunks occurs among the lists
    assert {int(W._cdiv(n, W.A_CHUNKS[name][1])) for n in lens if n} == set(range(1, W.A_CHUNKS[name][0] + 1))


# ---- B: scan carries ----
B_PASSES = {"B1": (2, 1025), "B2": (3, 2049), "B3": (2, 1200), "B4": (1, 1024), "B5": (2, 1025)}


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", sorted(W.B_KINDS))
def test_b_worlds_reach_the_scan_carries(name, metric):
    w = W.world(name, metric)
    lens = flat_lens(w)
    total = len(lens)
    nq = len(w.qv)
    assert w.dim >= 16
    for case in w.cases:
        nprobe, cand, _ = case
        pl = W.plan(w, nq, nprobe, cand)
        assert (pl.scan_passes, pl.n_ext) == B_PASSES[name]
        assert pl.list_chunks == 1
        for variant in ("filtered", "boost"):
            ref = W.reference(w, case, variant)
            probed = np.bincount(ref.probes.ravel(), minlength=total) > 0
            for m in range(1024, total + 1, 1024):
                for side in (np.arange(0, m), np.arange(m, total)):
                    if len(side):
                        assert (probed[side] & (lens[side] > 0)).any()
            if variant == "filtered":   # (unboosted: every edge list is its own query's first probe)
                for l in W.b_edge_lists(total):
                    assert probed[l] and lens[l] > 0, f"{name}: list {l}"
            # hits come from lists on both sides of 1024
            if total > 1024 and cand > 1:
                base = ref.list_base
                sides = set()
                for q in range(nq):
                    for f in ref.top[q]:
                        got = W.chunk_of(w, pl, f)
                        if got is not None:
                            sides.add(int(base[got[0]] + got[1]) >= 1024)
                assert sides == {False, True}
    if name == "B3":
        assert W.world_lists(w)[1] is not None and len(W.world_lists(w)[0].lens) == 600   # 1024: inside segment 1
    if name in ("B4", "B5"):
        assert W.world_lists(w)[1] is None and w.segs[1].n_docs > 0


# ---- C: coarse steps, assignment chunks ----
@pytest.mark.parametrize("metric", METRICS)
def test_c_world_reaches_the_coarse_steps(metric):
    w = W.world_c(metric)
    lens = flat_lens(w)
    nq = len(w.qv)
    assert len(lens) == W.C_LISTS >= 16257 and lens[-1] > 0
    for lo, hi in W.C_DUPS:
        assert np.array_equal(w.segs[0].cents[lo], w.segs[0].cents[hi])
        assert lens[hi] == 0 and lens[lo] == 2   # the lower list wins the rows of both
    n_rows = len(w.segs[0].vals)
    n_chunks, tpb = W.assign_chunks(n_rows, W.C_LISTS)
    assert n_chunks > 1 and tpb > 1
    assert all((lo // (128 * tpb)) != (hi // (128 * tpb)) for lo, hi in W.C_DUPS[:3])  # copies in different chunks
    assert len(w.small.vals) <= 64 and W.assign_chunks(len(w.small.vals), W.C_LISTS)[1] == 1
    for case in w.cases:
        nprobe, cand, _ = case
        pl = W.plan(w, nq, nprobe, cand)
        assert pl.coarse_steps == 2 and pl.coarse_tiles > 1 and pl.coarse_docs == (16384 - nprobe) // 128 * 128
        edge = pl.coarse_docs
        for variant in ("filtered", "boost"):
            ref = W.reference(w, case, variant)
            steps = [set((ref.probes[q] >= edge).tolist()) for q in range(nq)]
            if nprobe == 1:
                assert {True} in steps and {False} in steps
            else:
                assert sum(s == {False, True} for s in steps) >= 1, f"{case} {variant}"
        ref = filtered(w, case)
        for q, (lo, hi) in enumerate(W.C_DUPS):   # the duplicated centroid as a query: the lower copy first
            assert ref.probes[q, 0] == lo
            if nprobe >= 2:
                assert ref.probes[q, 1] == hi
        assert W.C_DUPS[0][0] < edge <= W.C_DUPS[0][1]   # one copy in each step


# ---- D: more items than workgroups ----
@pytest.mark.parametrize("metric", METRICS)
def test_d_world_has_more_items_than_workgroups(metric):
    w = W.world_d(metric)
    assert [l.lens.tolist() for l in W.world_lists(w)] == [l.lens.tolist() for l in W.world_lists(W.world("B2", metric))]
    nq = len(w.qv)
    assert nq == 128
    (case,) = w.cases
    pl = W.plan(w, nq, case[0], case[1])
    for variant in ("filtered", "boost"):
        ref = W.reference(w, case, variant)
        assert len(np.unique(ref.probes)) >= 1024
        assert W.count_items(w, ref, pl, nq) >= 1024


# ---- E: fold passes ----
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", sorted(W.E_KINDS))
def test_e_worlds_reach_the_fold_passes(name, metric):
    w = W.world(name, metric)
    n_lists, long_, uncl, nprobe = W.E_KINDS[name]
    nq = len(w.qv)
    assert nq == 9
    case = (nprobe, 64, 64)
    pl = W.plan(w, nq, nprobe, 64)
    assert pl.P == nprobe and pl.list_chunks == (4 if long_ else 1)
    assert pl.slots_q == nprobe * pl.list_chunks + pl.uncl_slots and pl.slots_q >= 256
    assert pl.fold_passes == W.E_PASSES[name]
    assert pl.fold_keys % 64 == 0   # (cand 64: a slot's keys lie in one pass)
    ref = filtered(w, case)
    assert (ref.probes[:, -1] == n_lists - 1).all()   # the last list is every query's last probe
    want = set(range(pl.fold_passes)) if not uncl else {0, pl.fold_passes - 1}
    for q in range(nq):
        passes = {W.slot_of(w, ref, pl, q, f) * 64 // pl.fold_keys for f in ref.top[q]}
        assert passes >= want, f"{name} q{q}: the best docs lie in passes {passes}"
    if uncl:   # without the filter too: the unclustered segment's slots come last
        ref = W.reference(w, case, "boost")
        for q in np.nonzero(w.boost == 1.0)[0]:
            passes = {W.slot_of(w, ref, pl, q, f) * 64 // pl.fold_keys for f in ref.top[q]}
            assert {0, pl.fold_passes - 1} <= passes


# ---- F: unclustered chunking ----
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", sorted(W.F_ORDERS))
def test_f_worlds_reach_the_unclustered_cap(name, metric):
    w = W.world(name, metric)
    assert W.uncl_chunking(4096) == (128, 32) and W.uncl_chunking(4097) == (256, 17)
    assert 4097 - 16 * 256 == 1   # the last slot of the larger segment holds one doc
    assert [s.n_docs for s in w.segs[1:]] == list(W.F_ORDERS[name])
    nq = len(w.qv)
    doc_base = np.cumsum([0] + [s.n_docs for s in w.segs])
    last = [int(doc_base[2]) - 1, int(doc_base[3]) - 1]
    for case in w.cases:
        pl = W.plan(w, nq, case[0], case[1])
        assert pl.uncl == [W.uncl_chunking(n) for n in W.F_ORDERS[name]] and pl.uncl_slots == 49
        assert pl.slots_q == pl.P + 49 and pl.n_ext == 8 + 2
        ref = filtered(w, case)
        for q in range(nq):
            assert set(last) <= set(ref.top[q].tolist()), f"{name} {case} q{q}"
            assert W.slot_of(w, ref, pl, q, last[1]) == pl.slots_q - 1   # the second segment's slots start past 0


# ---- G: build ranges ----
@pytest.mark.parametrize("metric", METRICS)
def test_g1_world_reaches_the_build_ranges(metric):
    w = W.world_g1(metric)
    assert [s.n_docs for s in w.segs] == [4096, 4097, 8255]
    assert [W.build_ranges(s.n_docs, 5) for s in w.segs] == [(4096, 1), (4096, 2), (4096, 3)]
    for s, l in zip(w.segs, W.world_lists(w)):
        assert int((s.offs == W.NOVEC).sum()) == s.n_docs // 4
        assert int(l.begin[-1]) == s.n_docs - s.n_docs // 4 and (l.lens > 0).all()
    assert 4097 % 4096 % 64 == 1 and 8255 % 4096 % 64 == 63   # the last wave of the last range is partly filled
    for r0 in (4096, 8192):   # docs without a vector on both sides of a range boundary
        assert (w.segs[2].offs[r0 - 64:r0] == W.NOVEC).any() and (w.segs[2].offs[r0:r0 + 64] == W.NOVEC).any()


def test_g2_world_reaches_the_longer_ranges():
    assert W.build_ranges(256 * 4096, 8) == (4096, 256)
    assert W.build_ranges(W.G2_DOCS, 8) == (4160, 253)
    offs, vals, begin, docs = W.world_g2()
    assert len(offs) == W.G2_DOCS and int(begin[-1]) == len(vals) == len(docs)
    assert (np.diff(begin.astype(np.int64)) > 0).all()
    assert np.array_equal(vals, np.round(vals)) and (vals == 5.0).any()   # 5: as near 0 as 10, the lower list's
    l0 = docs[begin[0]:begin[1]]
    assert (vals[offs[l0], 0] <= 5.0).all() and (vals[offs[l0], 0] == 5.0).any()
