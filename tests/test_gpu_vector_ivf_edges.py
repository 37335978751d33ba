"""The IVF calls at the scale their edge code exists for: list chunks, scan carries past 1024 lists, a second coarse
step, more items than workgroups, several fold passes, the unclustered chunk cap and several build ranges.

The worlds and the reference are tests/ivf_edge_worlds.py: grid-valued data whose scores are exact in f32, so a plain
numpy restatement of the call gives the device's bytes, and the lists, docs, segments, vector-score bytes, counts and
totals are compared without a tolerance.  tests/test_ivf_edge_worlds.py proves on the host that each world reaches its
edge.  Where it stays cheap the six outputs are also compared with the exact call under the membership filter of
tests/test_gpu_vector_ivf.py."""
import numpy as np
import pytest

from tests import ivf_edge_worlds as W
from tests.test_gpu_vector_ivf import Members, cents_of, centroid_index, probed_lists, same, seg_of
from tests.test_gpu_vector_search import _store, blend_rows, check

pytestmark = pytest.mark.gpu
F32 = np.float32


def segments(w):
    out = []
    for s in w.segs:
        g = seg_of(s.n_docs, (w.metric, s.offs, s.vals))
        if len(s.deleted):
            g.set_deleted([int(d) for d in s.deleted])
        out.append(g)
    return out


def open_index(w):
    import searchlite_amd as sa
    ix = sa.GpuIndex(segments(w))
    ix.cluster_vector_field(0, [s.cents for s in w.segs])
    return ix


def lists_agree(got, begin, docs, cents, what):
    assert got is not None, f"{what}: no lists"
    assert np.array_equal(got[0], begin), \
        f"{what}: list_begin differs first at list {np.nonzero(got[0] != begin)[0][:1]}"
    assert np.array_equal(got[1], docs), f"{what}: docs differ first at {np.nonzero(got[1] != docs)[0][:1]}"
    assert got[2].tobytes() == np.ascontiguousarray(cents, F32).tobytes(), f"{what}: centroids"


def world_lists_agree(ix, w):
    for si, (s, l) in enumerate(zip(w.segs, W.world_lists(w))):
        got = ix.fetch_vector_lists(0, si, w.dim)
        if l is None:
            assert got is None
        else:
            lists_agree(got, l.begin, l.docs, s.cents, f"{w.name} metric {w.metric} segment {si}")


def agrees(got, ref, what):
    doc, seg, _, vec, count, total = got
    for name, a, b in (("count", count, ref.count), ("total", total, ref.total)):
        bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, f"{what}: {name} of query {bad[0]}: {a[bad[0]]} != {b[bad[0]]} ({len(bad)} queries)"
    for name, a, b in (("seg", seg, ref.seg), ("doc", doc, ref.doc), ("vec", vec.view(np.uint32), ref.vec.view(np.uint32))):
        bad = np.nonzero(a != b)
        assert len(bad[0]) == 0, (f"{what}: {name} of query {bad[0][0]} row {bad[1][0]}: {a[bad[0][0], bad[1][0]]} != "
                                  f"{b[bad[0][0], bad[1][0]]} ({len(bad[0])} rows of {len(set(bad[0].tolist()))} queries)")


def ivf(ix, w, case, variant, q_filter):
    nprobe, cand, k_out = case
    if variant == "filtered":
        return ix.vector_search_ivf([0], w.qv, 0.0, cand, nprobe, k_out, q_filter=q_filter)
    return ix.vector_search_ivf([0], w.qv, 0.0, cand, nprobe, k_out, boost=w.boost.reshape(-1, 1))


def probe_sets(ref):
    base = ref.list_base
    seg = np.searchsorted(base, ref.probes, side="right") - 1
    return [frozenset((int(s), int(l - base[s])) for s, l in zip(seg[q], ref.probes[q])) for q in range(len(seg))]


# the worlds whose outputs are also compared with the exact call under the membership filter, and the case
EXACT_TOO = {"A1": (2, 33, 33), "B4": (4, 33, 33), "F1": (2, 64, 64), "G1": (2, 20, 20)}


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("name", W.SEARCH_WORLDS)
def test_lists_and_search_against_the_host_reference(name, metric):
    import torch
    w = W.world(name, metric)
    nq = len(w.qv)
    with open_index(w) as ix:
        world_lists_agree(ix, w)
        own_ids = [ix.add_filter(m) for m in w.own]
        q_filter = np.array([own_ids[o] if o >= 0 else -1 for o in w.own_of_query], np.int32)
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        for case in w.cases:
            for variant in ("filtered", "boost"):
                ref = W.reference(w, case, variant)
                if name == "D":   # more items than the launch has workgroups: two per CU at the most
                    items = W.count_items(w, ref, W.plan(w, nq, case[0], case[1]), nq)
                    assert items > 2 * n_cu, (items, n_cu)
                agrees(ivf(ix, w, case, variant, q_filter), ref, f"{name} metric {metric} {case} {variant}")
        if name == "C":
            assert W.assign_chunks(len(w.segs[0].vals), W.C_LISTS, n_cu)[0] > 1
        if name in EXACT_TOO:
            case = EXACT_TOO[name]
            mem = Members(ix, 0, [(metric, s.offs, s.vals) for s in w.segs], w.dim)
            for variant in ("filtered", "boost"):
                flt = variant == "filtered"
                ids = mem.filter_ids(probe_sets(W.reference(w, case, variant)), w.own, w.own_of_query if flt else None)
                want = ix.vector_search([0], w.qv, 0.0, case[1], case[2], q_filter=ids,
                                        boost=None if flt else w.boost.reshape(-1, 1))
                same(ivf(ix, w, case, variant, q_filter), want, f"{name} metric {metric} {case} {variant}")


@pytest.mark.parametrize("metric", [0, 1])
def test_a_store_of_one_query_tile_over_the_coarse_world_centroids(metric):
    """at most 64 rows: the assignment runs one workgroup per tile of 128 centroids and takes the best of 128 partials"""
    import searchlite_amd as sa
    s = W.world_c(metric).small
    begin, docs = W.build_lists(s.offs, W.assign_rows(metric, s.vals, s.cents), len(s.cents))
    with sa.GpuIndex([seg_of(s.n_docs, (metric, s.offs, s.vals))]) as ix:
        ix.cluster_vector_field(0, [s.cents])
        lists_agree(ix.fetch_vector_lists(0, 0, s.vals.shape[1]), begin, docs, s.cents, f"small store, metric {metric}")


def test_lists_of_1048577_docs():
    """past 256 ranges of 4096 docs: the ranges grow to 4160"""
    import searchlite_amd as sa
    offs, vals, begin, docs = W.world_g2()
    with sa.GpuIndex([seg_of(len(offs), (1, offs, vals))]) as ix:
        ix.cluster_vector_field(0, [W.G2_CENTS])
        lists_agree(ix.fetch_vector_lists(0, 0, 1), begin, docs, W.G2_CENTS, "1 048 577 docs")


# ---- two clauses: a small field's work area is laid out afresh after the chunked field's, and before it ----
@pytest.mark.parametrize("clause_field", [[0, 1], [1, 0]])
def test_two_clauses_a_small_field_beside_the_chunked_one(clause_field):
    w = W.world_a("A1", 0)
    s = w.segs[0]
    rng = np.random.default_rng(81)
    st1 = _store(rng, s.n_docs, 5, 1)
    c1 = np.ascontiguousarray(st1[2][rng.choice(len(st1[2]), 4, replace=False)])
    fields, cents, metrics, dims = [[(0, s.offs, s.vals)], [st1]], [[s.cents], [c1]], [0, 1], [w.dim, 5]
    nq, nprobe, cand, k_out = 9, 2, 12, 15
    parts = [w.qv[[0, 1, 2, 64, 129, 130, 133, 137, 141]], rng.standard_normal((nq, 5)).astype(F32)]
    qv = np.concatenate([parts[f] for f in clause_field], axis=1)
    alpha = np.zeros((nq, 2), F32)
    alpha[1], alpha[2], alpha[3, 0], alpha[4] = 1.0, 0.3, 0.75, [0.0, 1.0]
    boost = np.ones((nq, 2), F32)
    boost[5], boost[6, 0], boost[7, 1] = 1.5, -2.0, 0.0
    with open_index(w) as ix:
        assert ix.add_vector_field(fields[1]) == 1
        ix.cluster_vector_field(1, cents[1])
        got = ix.vector_search_ivf(clause_field, qv, alpha, cand, nprobe, k_out, boost=boost)
        maps = [[] for _ in range(nq)]
        for c, f in enumerate(clause_field):
            qc, bc = np.ascontiguousarray(parts[f]), np.ascontiguousarray(boost[:, c:c + 1])
            with centroid_index(cents_of(fields[f], cents[f]), metrics[f]) as cix:
                probes = probed_lists(cix, qc, bc, nprobe)
            ids = Members(ix, f, fields[f], dims[f]).filter_ids(probes)
            doc, seg, _, vec, cnt, _ = ix.vector_search([f], qc, 0.0, cand, cand, boost=bc, q_filter=ids)
            for q in range(nq):
                maps[q].append({(int(seg[q, i]), int(doc[q, i])): F32(vec[q, i]) for i in range(int(cnt[q]))})
        want = []
        for q in range(nq):
            rows, total = blend_rows(maps[q], metrics, clause_field, alpha[q], k_out)
            want.append((rows, total, maps[q]))
        check(got, want, k_out, f"fields {clause_field}")
        for q in range(nq):
            assert int(got[5][q]) == want[q][1]


# ---- the device form, over the world with more items than workgroups ----
@pytest.mark.parametrize("metric", [0, 1])
def test_device_form_is_the_host_form(metric):
    import torch
    w = W.world_d(metric)
    nq = len(w.qv)
    (case,) = w.cases
    nprobe, cand, k_out = case
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with open_index(w) as ix:
        own_ids = [ix.add_filter(m) for m in w.own]
        q_filter = np.array([own_ids[o] if o >= 0 else -1 for o in w.own_of_query], np.int32)
        boost = w.boost.reshape(-1, 1)
        host = ix.vector_search_ivf([0], w.qv, 0.0, cand, nprobe, k_out, boost=boost, q_filter=q_filter)
        dq, da, db, df = t(w.qv), t(np.zeros((nq, 1), F32)), t(boost), t(q_filter)
        od = torch.zeros((nq, k_out), dtype=torch.int32, device=dev)
        os_, osc, ov = torch.zeros_like(od), torch.zeros((nq, k_out), device=dev), torch.zeros((nq, k_out), device=dev)
        oc = torch.zeros(nq, dtype=torch.int32, device=dev)
        ot = torch.zeros(nq, dtype=torch.int64, device=dev)
        ix.vector_search_ivf_device(nq, [0], dq.data_ptr(), da.data_ptr(), db.data_ptr(), df.data_ptr(), cand, nprobe,
                                    k_out, od.data_ptr(), os_.data_ptr(), osc.data_ptr(), ov.data_ptr(), oc.data_ptr(),
                                    ot.data_ptr())
        torch.cuda.synchronize()
        same([x.cpu().numpy() for x in (od, os_, osc, ov, oc, ot)], host, f"device form, metric {metric}")
        assert int(host[4].max()) > 0


# ---- training past 1024 lists and past one build range ----
@pytest.mark.parametrize("iters", [1, 2])   # (2: the first step that compares two assignments, vs_ivf_moved_kernel)
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("name", ["B2", "G1"])
def test_training_gives_the_lists_of_its_centroids(name, metric, iters):
    """The centroids a step leaves are no longer grid-valued, so the test asserts that no such centroid scores within
    1e-3 (far more than an f32 rounding) of a row's best other centroid: then the float64 assignment is the device's."""
    import searchlite_amd as sa
    w = W.world(name, metric)
    # cosine: a step leaves unit centroids, and an empty list keeps its start; at half the world's length (0.87) a kept
    # start scores below every unit centroid's own rows, as the world's own centroids (1.73) would not
    inits = [s.cents * F32(0.5) if metric == 0 else s.cents for s in w.segs]
    with sa.GpuIndex(segments(w)) as ix:
        stats = ix.train_vector_field(0, [(len(c), iters, c) for c in inits])
        for si, s in enumerate(w.segs):
            assert stats[si]["iters_run"] >= 1
            begin, docs, cents = ix.fetch_vector_lists(0, si, w.dim)
            assert not np.array_equal(cents, inits[si])
            trained = (cents.view(np.uint32) != inits[si].view(np.uint32)).any(axis=1)
            row_list = np.empty(len(s.vals), np.int64)
            for r0 in range(0, len(s.vals), 1024):
                sc = W.scores(metric, s.vals[r0:r0 + 1024], cents)
                row_list[r0:r0 + 1024] = np.argmax(W.order_key(sc), axis=1)   # (the first of equal scores)
                # a centroid that a step left is not grid-valued: its score must not lie near a row's best one, unless
                # it is the only one there (centroids that kept their start score exactly, and may tie)
                near = sc.astype(np.float64) >= sc.max(axis=1, keepdims=True).astype(np.float64) - 1e-3
                crowded = near.sum(axis=1) > 1
                assert not (near[crowded] & trained[None, :]).any(), "a trained centroid nearly ties for a row"
            want_begin, want_docs = W.build_lists(s.offs, row_list, len(cents))
            lists_agree((begin, docs, cents), want_begin, want_docs, cents, f"{name} metric {metric} segment {si}")
            assert stats[si]["max_len"] == int(np.diff(want_begin.astype(np.int64)).max())
