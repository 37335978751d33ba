"""IVF vector search on the device (slg_index_cluster_vector_field, slg_vector_search_batch_ivf*) against the exact
call itself, slg_vector_search_batch, through two references built from the public interface:

  the centroid index: a second GpuIndex with one segment per segment of the index under test, whose docs are that
    segment's lists and whose vectors are its centroids (an unclustered or vector-less segment: one doc without a
    vector).  The exact call over it with a segment's rows as queries, cand_size 1, names the list of every row; with
    the test's queries and boosts, cand_size = the probes of a query, it names every query's probed lists.
  the membership filter: per query a registered bitmap, true on the docs of the query's probed lists (as
    fetch_vector_lists returns them) and on every doc of an unclustered segment, ANDed with the test's own filter.

Every score the IVF call returns is the exact call's bit for bit, so with one clause all six outputs must be
byte-identical to the exact call under the membership filter; several clauses are blended on the host (blend_rows)
and compared with check() at its own TOL."""
import numpy as np
import pytest

from tests.test_gpu_vector_approx import _fields_world
from tests.test_gpu_vector_search import NOVEC, _seg, _store, _unit, blend_rows, check

pytestmark = pytest.mark.gpu
F32 = np.float32


def same(got, want, what):
    for name, a, b in zip(("doc", "seg", "score", "vec", "count", "total"), got, want):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), \
            f"{what}: {name} differs from the exact call"


# ---- the two references ----
def centroid_index(cents, metric):
    """cents[s]: the centroids of segment s, or None (unclustered, or no vectors in the field)"""
    import searchlite_amd as sa
    return sa.GpuIndex([_seg(1) if c is None else _seg(len(c), np.arange(len(c)), c, metric) for c in cents])


def expected_lists(cix, s, store):
    """(list_begin, docs) of segment s's store around the centroid index's segment s"""
    _, offs, vals = store
    n_lists = cix.segments[s].n_docs
    fid = cix.add_filter([np.full(g.n_docs, t == s) for t, g in enumerate(cix.segments)])
    doc, seg, _, _, cnt, _ = cix.vector_search([0], vals, 1.0, 1, 1, q_filter=np.full(len(vals), fid, np.int32))
    assert (cnt == 1).all() and (seg[:, 0] == s).all()
    row_list = doc[:, 0]
    lists = [[] for _ in range(n_lists)]
    for d in range(len(offs)):
        if offs[d] != NOVEC:
            lists[int(row_list[offs[d]])].append(d)
    begin = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
    return begin, np.array([d for x in lists for d in x], np.uint32)


def probed_lists(cix, qv, boost, nprobe):
    """per query the set of (segment, list) the exact call over the centroid index keeps"""
    total = sum(g.n_docs for g in cix.segments if g.vec_dim)
    P = min(nprobe, total)
    doc, seg, _, _, cnt, _ = cix.vector_search([0], qv, 1.0, P, P, boost=boost)
    assert (cnt == P).all()
    return [frozenset((int(s), int(d)) for s, d in zip(seg[q], doc[q])) for q in range(len(qv))]


class Members:
    """registers, per distinct (probed set, own filter), the membership filter on the index under test"""

    def __init__(self, ix, field, stores, dim):
        self.ix, self.stores, self.known = ix, stores, {}
        self.lists = [ix.fetch_vector_lists(field, s, dim) for s in range(len(stores))]

    def filter_ids(self, probes, own_masks=None, own_of_query=None):
        ids = []
        for q, pr in enumerate(probes):
            own = -1 if own_of_query is None else int(own_of_query[q])
            if (pr, own) not in self.known:
                masks = []
                for s, st in enumerate(self.stores):
                    n = self.ix.segments[s].n_docs
                    if self.lists[s] is None:
                        m = np.ones(n, bool)  # (unclustered: scanned whole; without the field: nothing to score)
                    else:
                        begin, docs, _ = self.lists[s]
                        m = np.zeros(n, bool)
                        for (ps, pl) in pr:
                            if ps == s:
                                m[docs[begin[pl]:begin[pl + 1]]] = True
                    if own >= 0:
                        m &= own_masks[own][s]
                    masks.append(m)
                self.known[(pr, own)] = self.ix.add_filter(masks)
            ids.append(self.known[(pr, own)])
        return np.array(ids, np.int32)


def seg_of(n_docs, store):
    """a segment whose field-0 store is (metric, offsets, values), or without vectors (None)"""
    return _seg(n_docs) if store is None else _seg(n_docs, store[1], store[2], store[0])


def cents_of(stores, cents):
    return [c if st is not None else None for st, c in zip(stores, cents)]


# ---- 1. the lists, bit for bit ----
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("dim", [1, 7, 33, 100])
def test_lists_bit_for_bit(dim, metric):
    import searchlite_amd as sa
    rng = np.random.default_rng(100 * dim + metric)
    n0, n2 = 300, 90
    # cosine rows in the positive orthant, so that the centroid -1 / sqrt(dim) attracts nobody
    vals = np.abs(_unit(rng, n0, dim)) if metric == 0 else rng.standard_normal((n0, dim)).astype(F32)
    st0 = _store(rng, n0, dim, metric, values=vals)
    st2 = _store(rng, n2, dim, metric, values=vals[:n2].copy())
    rows = st0[2]
    far = np.full(dim, -1.0 / np.sqrt(dim) if metric == 0 else 1.0e3, F32)
    c = [rows[3], rows[3], far, rows[11], rows[20] * F32(0.5) + rows[21] * F32(0.5), rows[40]]
    if metric == 0:
        c.append(np.full(dim, np.nan, F32))  # its score is 0
    c.append(rows[7])
    cents = np.ascontiguousarray(np.stack(c), F32)
    stores = [st0, None, st2]
    with sa.GpuIndex([seg_of(n0, st0), _seg(50), seg_of(n2, st2)]) as ix, \
            centroid_index([cents, None, None], metric) as cix:
        ix.cluster_vector_field(0, [cents, None, None])
        begin, docs, got_c = ix.fetch_vector_lists(0, 0, dim)
        want_begin, want_docs = expected_lists(cix, 0, st0)
        assert np.array_equal(begin, want_begin) and np.array_equal(docs, want_docs), f"dim {dim} metric {metric}"
        assert got_c.tobytes() == cents.tobytes()
        lens = np.diff(begin.astype(np.int64))
        for l in range(len(cents)):
            assert np.all(np.diff(docs[begin[l]:begin[l + 1]].astype(np.int64)) > 0)
        assert lens[1] == 0 and lens[0] > 0      # two identical centroids: the lower id gets the docs
        assert lens[2] == 0                      # the far-away centroid: an empty list
        if dim > 1:
            assert st0[1][docs[begin[3]:begin[4]]].tolist().count(11) == 1  # the doc that is centroid 3
        if metric == 0:
            assert lens[6] == 0                  # NaN centroid: score 0 < every positive cosine
        assert int(begin[-1]) == int((st0[1] != NOVEC).sum())
        assert ix.fetch_vector_lists(0, 1, dim) is None   # a segment without the field
        assert ix.fetch_vector_lists(0, 2, dim) is None   # n_lists 0


# ---- the designed world of case 2: list lengths 0, 1, 127, 128, 129; lists probed by 0, 1, 63, 64, 65 queries ----
def _near(rng, c, n, metric, spread=0.02):
    v = c[None, :] + spread * rng.standard_normal((n, len(c))).astype(F32)
    if metric == 0:
        v = v / np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(F32)


def _designed(rng, metric, dim=33):
    sizes = [129, 128, 127, 1, 0, 40]
    if metric == 0:
        cents = np.eye(dim, dtype=F32)[:6].copy()
        cents[4] = -cents[[0, 1, 2, 3, 5]].sum(axis=0) / np.sqrt(F32(5))   # the farthest from every doc
    else:
        cents = (np.eye(dim, dtype=F32)[:6] * F32(10)).copy()
        cents[4] = F32(500)
    vals = np.concatenate([_near(rng, cents[l], n, metric) for l, n in enumerate(sizes) if n])
    n_rows = len(vals)
    n_docs = n_rows + 6
    have = np.ones(n_docs, bool)
    have[rng.choice(n_docs, 6, replace=False)] = False
    offs = np.full(n_docs, NOVEC, np.uint32)
    offs[np.nonzero(have)[0]] = rng.permutation(n_rows)
    # 63 queries nearest list 0 then 3, 64 nearest 1 then 5, 1 nearest 2 then 0, 2 nearest 5 then 3
    q = []
    for a, b, n in ((0, 3, 63), (1, 5, 64), (2, 0, 1), (5, 3, 2)):
        q.append(_near(rng, cents[a] + F32(0.4) * cents[b], n, metric, spread=0.01))
    return (metric, offs, vals), cents, sizes, np.concatenate(q)


def _boost(rng, nq, kind):
    if kind is None:
        return None
    b = np.ones((nq, 1), F32)
    if kind == "mixed":
        b[::3] = -1.5
        b[1::7] = 0.0
        b[2::5] = 2.25
    return b


DESIGNED_CASES = [(1, 1, 0, None), (1, 32, 40, "mixed"), (1, 64, 64, None), (2, 33, 34, "mixed"), (2, 64, 70, None),
                  (2, 5, 5, None), (5, 32, 33, "mixed"), (5, 1, 3, None)]


@pytest.mark.parametrize("metric", [0, 1])
def test_single_clause_partial_probes_designed_world(metric):
    import searchlite_amd as sa
    rng = np.random.default_rng(17 + metric)
    st, cents, sizes, qv = _designed(rng, metric)
    nq, dim, n_docs = len(qv), cents.shape[1], len(st[1])
    assert nq == 130
    seg = seg_of(n_docs, st)
    seg.set_deleted([2, 3, 50, 200, 201])
    own = [[rng.random(n_docs) < 0.6], [rng.random(n_docs) < 0.1]]
    with sa.GpuIndex([seg]) as ix, centroid_index([cents], metric) as cix:
        ix.cluster_vector_field(0, [cents])
        begin, docs, _ = ix.fetch_vector_lists(0, 0, dim)
        assert np.diff(begin.astype(np.int64)).tolist() == sizes
        own_ids = [ix.add_filter(m) for m in own]
        own_of_query = np.where(np.arange(nq) % 4 == 1, 0, np.where(np.arange(nq) % 9 == 2, 1, -1))
        q_filter = np.array([own_ids[o] if o >= 0 else -1 for o in own_of_query], np.int32)
        mem = Members(ix, 0, [st], dim)
        seen_counts = set()
        for nprobe, cand, k_out, bk in DESIGNED_CASES:
            boost = _boost(rng, nq, bk)
            probes = probed_lists(cix, qv, boost, nprobe)
            if bk is None:
                per_list = [sum((0, l) in p for p in probes) for l in range(6)]
                seen_counts.update(per_list)
            for filtered in (False, True):
                ids = mem.filter_ids(probes, own, own_of_query if filtered else None)
                want = ix.vector_search([0], qv, 0.0, cand, k_out, boost=boost, q_filter=ids)
                got = ix.vector_search_ivf([0], qv, 0.0, cand, nprobe, k_out, boost=boost,
                                           q_filter=q_filter if filtered else None)
                same(got, want, f"metric {metric} nprobe {nprobe} cand {cand} k_out {k_out} boost {bk} "
                                f"filtered {filtered}")
            assert k_out == 0 or int(want[4].max()) > 0
        assert {0, 1, 63, 64, 65} <= seen_counts, seen_counts
        # nq 1
        for nprobe in (1, 2, 5):
            probes = probed_lists(cix, qv[:1], None, nprobe)
            same(ix.vector_search_ivf([0], qv[:1], 0.0, 10, nprobe, 10),
                 ix.vector_search([0], qv[:1], 0.0, 10, 10, q_filter=mem.filter_ids(probes)), f"nq 1 nprobe {nprobe}")


# ---- case 2, several segments: different n_lists, an unclustered segment, a segment without the field, the
#      (segment, list) tie rule with duplicated centroids ----
def _segments_world(rng, metric, dim):
    n_docs = [230, 140, 50, 310]
    mk = lambda n: (np.abs(_unit(rng, n, dim)) if metric == 0 else rng.standard_normal((n, dim)).astype(F32))
    stores = [_store(rng, n_docs[0], dim, metric, values=mk(n_docs[0])),
              _store(rng, n_docs[1], dim, metric, values=mk(n_docs[1])), None,
              _store(rng, n_docs[3], dim, metric, values=mk(n_docs[3]))]
    a = stores[0][2][5]
    cents = [np.stack([a, a, stores[0][2][9]]), None, None,
             np.stack([a, stores[3][2][1], stores[3][2][2], stores[3][2][3], stores[3][2][4]])]
    return n_docs, stores, [np.ascontiguousarray(c, F32) if c is not None else None for c in cents]


@pytest.mark.parametrize("metric,dim", [(0, 7), (1, 7), (0, 100), (1, 33)])
def test_single_clause_partial_probes_several_segments(metric, dim):
    import searchlite_amd as sa
    rng = np.random.default_rng(1000 * metric + dim)
    n_docs, stores, cents = _segments_world(rng, metric, dim)
    segs = [seg_of(n, st) for n, st in zip(n_docs, stores)]
    segs[3].set_deleted([0, 7, 300])
    nq = 37
    qv = np.abs(_unit(rng, nq, dim)) if metric == 0 else rng.standard_normal((nq, dim)).astype(F32)
    qv[0] = stores[0][2][5]  # the duplicated centroid itself: its three lists tie, (segment, list) decides
    own = [[rng.random(n) < 0.5 for n in n_docs]]
    with sa.GpuIndex(segs) as ix, centroid_index(cents, metric) as cix:
        ix.cluster_vector_field(0, cents)
        bits = np.zeros(n_docs[0], bool)
        bits[[1, 2, 100]] = True
        ix.update_deleted(0, np.packbits(bits, bitorder="little"), float(n_docs[0] - 3))
        own_id = ix.add_filter(own[0])
        own_of_query = np.where(np.arange(nq) % 3 == 0, 0, -1)
        q_filter = np.where(own_of_query >= 0, own_id, -1).astype(np.int32)
        mem = Members(ix, 0, stores, dim)
        assert mem.lists[1] is None and mem.lists[2] is None and len(mem.lists[0][0]) == 4 and len(mem.lists[3][0]) == 6
        total = 8
        for nprobe, cand, k_out, bk in ((1, 33, 40, None), (1, 8, 8, "mixed"), (2, 64, 64, None), (2, 1, 1, "mixed"),
                                        (total - 1, 32, 0, None), (total - 1, 20, 25, "mixed")):
            boost = _boost(rng, nq, bk)
            probes = probed_lists(cix, qv, boost, nprobe)
            if bk is None and nprobe <= 2:
                want0 = {(0, 0)} if nprobe == 1 else {(0, 0), (0, 1)}
                assert probes[0] == want0, probes[0]  # the tie rule: segment asc, then list asc
            for filtered in (False, True):
                ids = mem.filter_ids(probes, own, own_of_query if filtered else None)
                want = ix.vector_search([0], qv, 0.0, cand, k_out, boost=boost, q_filter=ids)
                got = ix.vector_search_ivf([0], qv, 0.0, cand, nprobe, k_out, boost=boost,
                                           q_filter=q_filter if filtered else None)
                same(got, want, f"metric {metric} dim {dim} nprobe {nprobe} cand {cand} boost {bk} filtered {filtered}")
            # the unclustered segment is scanned whole: its docs show up whatever is probed
            if k_out and bk is None:
                assert any((want[1][q, :int(want[4][q])] == 1).any() for q in range(nq))


# ---- 3. all lists probed: the exact call, several clauses ----
FDIMS, FMETRICS = [36, 100, 257, 5], [0, 1, 0, 1]


def _cluster_fields(rng, ix, fields, ks=(4, 3, 5, 6)):
    """cluster every field of _fields_world around rows of its own stores -> cents[f][s]"""
    all_cents = []
    for f, per_seg in enumerate(fields):
        cents = []
        for s, st in enumerate(per_seg):
            k = ks[(f + s) % len(ks)]
            cents.append(None if st is None else np.ascontiguousarray(st[2][rng.choice(len(st[2]), k, replace=False)]))
        ix.cluster_vector_field(f, cents)
        all_cents.append(cents)
    return all_cents


def _world_queries(rng, clause_field, nq):
    nc = len(clause_field)
    qv = np.concatenate([_unit(rng, nq, FDIMS[f]) if FMETRICS[f] == 0 else
                         rng.standard_normal((nq, FDIMS[f])).astype(F32) for f in clause_field], axis=1)
    alpha = np.zeros((nq, nc), F32)
    alpha[1], alpha[2], alpha[3, 0] = 1.0, 0.3, 0.75
    alpha[4] = np.linspace(0.0, 1.0, nc, dtype=F32)
    boost = np.ones((nq, nc), F32)
    boost[5], boost[6, 0], boost[7, nc - 1] = 1.5, -2.0, 0.0
    return qv, alpha, boost


@pytest.mark.parametrize("clause_field", [[0], [3], [2], [1, 0], [0, 3, 1]])
def test_all_lists_probed_is_the_exact_call(clause_field):
    import searchlite_amd as sa
    rng = np.random.default_rng(31 * len(clause_field) + clause_field[0])
    n_docs = (260, 180)
    fields = _fields_world(rng, n_docs, FDIMS, FMETRICS)
    qv, alpha, boost = _world_queries(rng, clause_field, 9)
    segs = [seg_of(n, fields[0][s]) for s, n in enumerate(n_docs)]
    segs[0].set_deleted([1, 5, 17])
    with sa.GpuIndex(segs) as ix:
        for f in (1, 2, 3):
            assert ix.add_vector_field(fields[f]) == f
        cents = _cluster_fields(rng, ix, fields)
        most = max(sum(len(c) for c in cents[f] if c is not None) for f in clause_field)
        for cand, k_out in ((10, 13), (64, 64), (1, 2)):
            want = ix.vector_search(clause_field, qv, alpha, cand, k_out, boost=boost)
            for nprobe in (most, 256):
                got = ix.vector_search_ivf(clause_field, qv, alpha, cand, nprobe, k_out, boost=boost)
                same(got, want, f"fields {clause_field} cand {cand} nprobe {nprobe}")


# ---- 4. several clauses, partial probes: per-clause lists from the exact call, blended on the host ----
@pytest.mark.parametrize("clause_field,nprobe", [([1, 0], 2), ([0, 3, 1], 1), ([0, 3, 1], 3), ([2, 0], 2)])
def test_several_clauses_partial_probes(clause_field, nprobe):
    import searchlite_amd as sa
    rng = np.random.default_rng(97 * len(clause_field) + nprobe)
    n_docs = (260, 180)
    fields = _fields_world(rng, n_docs, FDIMS, FMETRICS)
    nq, nc, cand, k_out = 9, len(clause_field), 12, 15
    qv, alpha, boost = _world_queries(rng, clause_field, nq)
    offs = np.concatenate([[0], np.cumsum([FDIMS[f] for f in clause_field])])
    segs = [seg_of(n, fields[0][s]) for s, n in enumerate(n_docs)]
    with sa.GpuIndex(segs) as ix:
        for f in (1, 2, 3):
            assert ix.add_vector_field(fields[f]) == f
        cents = _cluster_fields(rng, ix, fields)
        got = ix.vector_search_ivf(clause_field, qv, alpha, cand, nprobe, k_out, boost=boost)
        maps = [[] for _ in range(nq)]
        for c, f in enumerate(clause_field):
            qc = np.ascontiguousarray(qv[:, offs[c]:offs[c + 1]])
            bc = np.ascontiguousarray(boost[:, c:c + 1])
            with centroid_index(cents_of(fields[f], cents[f]), FMETRICS[f]) as cix:
                probes = probed_lists(cix, qc, bc, nprobe)
            ids = Members(ix, f, fields[f], FDIMS[f]).filter_ids(probes)
            doc, seg, _, vec, cnt, _ = ix.vector_search([f], qc, 0.0, cand, cand, boost=bc, q_filter=ids)
            for q in range(nq):
                maps[q].append({(int(seg[q, i]), int(doc[q, i])): F32(vec[q, i]) for i in range(int(cnt[q]))})
        want = []
        for q in range(nq):
            rows, total = blend_rows(maps[q], FMETRICS, clause_field, alpha[q], k_out)
            want.append((rows, total, maps[q]))
        check(got, want, k_out, f"fields {clause_field} nprobe {nprobe}")
        for q in range(nq):
            assert int(got[5][q]) == want[q][1]


# ---- 5. lifecycle ----
def test_lifecycle():
    import searchlite_amd as sa
    from searchlite_amd import _native as N
    rng = np.random.default_rng(77)
    dim, metric = 40, 0
    n_docs = [300, 200]
    stores = [_store(rng, n, dim, metric) for n in n_docs]
    cents = [np.ascontiguousarray(st[2][rng.choice(len(st[2]), k, replace=False)]) for st, k in zip(stores, (5, 3))]
    nq, cand, k_out = 11, 15, 16
    qv = _unit(rng, nq, dim)

    def both(ix, cents_now, stores_now, nprobe, what):
        with centroid_index(cents_of(stores_now, cents_now), metric) as cix:
            probes = probed_lists(cix, qv, None, nprobe)
        ids = Members(ix, 0, stores_now, dim).filter_ids(probes)
        want = ix.vector_search([0], qv, 0.2, cand, k_out, q_filter=ids)
        got = ix.vector_search_ivf([0], qv, 0.2, cand, nprobe, k_out)
        same(got, want, what)
        return got

    def lists_bytes(ix, s):
        got = ix.fetch_vector_lists(0, s, dim)
        return None if got is None else tuple(a.tobytes() for a in got)

    with sa.GpuIndex([seg_of(n, st) for n, st in zip(n_docs, stores)]) as ix:
        ix.cluster_vector_field(0, cents)
        got = both(ix, cents, stores, 2, "clustered")
        before = [lists_bytes(ix, s) for s in range(2)]
        # tombstones after clustering: the results follow them, the lists stay
        bits = np.zeros(300, bool)
        bits[[int(d) for q in range(nq) for d, s in zip(got[0][q, :3], got[1][q, :3]) if s == 0] + [1, 2]] = True
        ix.update_deleted(0, np.packbits(bits, bitorder="little"), float(300 - bits.sum()))
        assert [lists_bytes(ix, s) for s in range(2)] == before
        after = both(ix, cents, stores, 2, "update_deleted")
        assert not np.array_equal(after[0], got[0])
        # a new segment is unclustered and scanned whole
        st2 = _store(rng, 150, dim, metric)
        assert ix.add_segment(seg_of(150, st2)) == 2
        assert ix.fetch_vector_lists(0, 2, dim) is None
        assert [lists_bytes(ix, s) for s in range(2)] == before
        got = both(ix, cents + [None], stores + [st2], 2, "add_segment")
        assert (got[1] == 2).any()
        # a batch prepared now runs on this state after the re-cluster below
        q1 = np.ascontiguousarray(qv[:1])
        with ix.prepare(np.array([0, 1], np.uint32), np.zeros((1, 3), np.uint32), np.ones(1, F32), 5,
                        hybrid=True) as b:  # (term 0 of each of the three segments)
            hy_before = b.hybrid([0], q1, 0.5, 5, 5)
            # cluster only the new segment: the old ones keep their lists by reference
            c2 = np.ascontiguousarray(st2[2][rng.choice(len(st2[2]), 4, replace=False)])
            ix.cluster_vector_field(0, [N.KEEP_VECTOR_LISTS, N.KEEP_VECTOR_LISTS, c2])
            hy_after = b.hybrid([0], q1, 0.5, 5, 5)
            same(hy_after, hy_before, "a hybrid batch prepared before the re-cluster")
        assert [lists_bytes(ix, s) for s in range(2)] == before
        with centroid_index([None, None, c2], metric) as cix:
            want_begin, want_docs = expected_lists(cix, 2, st2)
        begin, docs, cc = ix.fetch_vector_lists(0, 2, dim)
        assert np.array_equal(begin, want_begin) and np.array_equal(docs, want_docs) and cc.tobytes() == c2.tobytes()
        both(ix, cents + [c2], stores + [st2], 3, "re-clustered")
        # KEEP where there is nothing to keep: unclustered stays unclustered; n_lists 0 unclusters
        ix.cluster_vector_field(0, [N.KEEP_VECTOR_LISTS, None, N.KEEP_VECTOR_LISTS])
        assert lists_bytes(ix, 0) == before[0] and lists_bytes(ix, 1) is None and lists_bytes(ix, 2) is not None
        ix.cluster_vector_field(0, [N.KEEP_VECTOR_LISTS, N.KEEP_VECTOR_LISTS, N.KEEP_VECTOR_LISTS])
        assert lists_bytes(ix, 1) is None
        both(ix, [cents[0], None, c2], stores + [st2], 2, "segment 1 unclustered again")
        # remove_segment drops that segment's lists, the others keep theirs
        kept = lists_bytes(ix, 2)
        ix.remove_segment(0)
        assert lists_bytes(ix, 0) is None and lists_bytes(ix, 1) == kept
        both(ix, [None, c2], [stores[1], st2], 1, "remove_segment")


# ---- 6. the _device form ----
def test_device_form_is_the_host_form_and_leaves_nothing_behind():
    import torch
    import searchlite_amd as sa
    rng = np.random.default_rng(5)
    dim, d1 = 36, 5
    n_docs = [400, 250]
    f0 = [_store(rng, n, dim, 0) for n in n_docs]
    f1 = [_store(rng, n_docs[0], d1, 1), None]
    c0 = [np.ascontiguousarray(st[2][rng.choice(len(st[2]), k, replace=False)]) for st, k in zip(f0, (7, 4))]
    c1 = [np.ascontiguousarray(f1[0][2][rng.choice(len(f1[0][2]), 6, replace=False)]), None]
    nq, cand, k_out = 70, 20, 21
    qv = np.concatenate([_unit(rng, nq, dim), rng.standard_normal((nq, d1)).astype(F32)], axis=1)
    boost = np.full((nq, 2), 1.5, F32)
    boost[::4, 1] = -1.0
    flt_mask = [rng.random(n) < 0.7 for n in n_docs]

    def index():
        ix = sa.GpuIndex([seg_of(n, st) for n, st in zip(n_docs, f0)])
        assert ix.add_vector_field(f1) == 1
        ix.cluster_vector_field(0, c0)
        ix.cluster_vector_field(1, c1)
        assert ix.add_filter(flt_mask) == 0
        return ix
    q_filter = np.where(np.arange(nq) % 2 == 0, 0, -1).astype(np.int32)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dq, da, db, df = t(qv), t(np.full((nq, 2), 0.2, F32)), t(boost), t(q_filter)

    def device_call(ix, nprobe):
        od = torch.zeros((nq, k_out), dtype=torch.int32, device=dev)
        os_, osc, ov = torch.zeros_like(od), torch.zeros((nq, k_out), device=dev), torch.zeros((nq, k_out), device=dev)
        oc = torch.zeros(nq, dtype=torch.int32, device=dev)
        ot = torch.zeros(nq, dtype=torch.int64, device=dev)
        ix.vector_search_ivf_device(nq, [0, 1], dq.data_ptr(), da.data_ptr(), db.data_ptr(), df.data_ptr(), cand,
                                    nprobe, k_out, od.data_ptr(), os_.data_ptr(), osc.data_ptr(), ov.data_ptr(),
                                    oc.data_ptr(), ot.data_ptr())
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in (od, os_, osc, ov, oc, ot)]

    with index() as fresh:
        fresh_1 = device_call(fresh, 1)
    with index() as ix:
        for nprobe in (11, 1, 3):  # all lists first, then one: nothing of the first call is left over
            host = ix.vector_search_ivf([0, 1], qv, 0.2, cand, nprobe, k_out, boost=boost, q_filter=q_filter)
            got = device_call(ix, nprobe)
            same(got, host, f"device form, nprobe {nprobe}")
            if nprobe == 1:
                same(got, fresh_1, "nprobe 1 after nprobe = total against a fresh index")
        assert not np.array_equal(fresh_1[0], device_call(ix, 11)[0])


# ---- 7. error codes, then a valid call ----
def test_error_codes_then_a_valid_call():
    import ctypes as C
    import searchlite_amd as sa
    from searchlite_amd import _native as N
    rng = np.random.default_rng(3)
    dim = 8
    stores = [_store(rng, 100, dim, 0), None]
    qv = _unit(rng, 2, dim)
    cents = np.ascontiguousarray(stores[0][2][:3])
    lib = N.load()
    with sa.GpuIndex([seg_of(100, stores[0]), _seg(20)]) as ix:
        def rc(fn, *a, **kw):
            try:
                fn(*a, **kw)
            except N.SlgError as e:
                return e.code, str(e)
            return 0, ""
        code, msg = rc(ix.vector_search_ivf, [0], qv, 0.0, 5, 2, 3)
        assert code == N.ERR_INVALID and "field 0" in msg                        # no lists yet
        ix.cluster_vector_field(0, [None, None])                                  # ... and none after this
        code, msg = rc(ix.vector_search_ivf, [0], qv, 0.0, 5, 2, 3)
        assert code == N.ERR_INVALID and "field 0" in msg
        assert rc(ix.cluster_vector_field, 1, [cents, None])[0] == N.ERR_INVALID  # no such field
        assert rc(ix.cluster_vector_field, 0, [cents])[0] == N.ERR_INVALID        # n_segs mismatch
        assert rc(ix.cluster_vector_field, 0, [cents, None, None])[0] == N.ERR_INVALID
        assert rc(ix.cluster_vector_field, 0, [None, cents])[0] == N.ERR_INVALID  # a segment without vectors
        d = (N.VectorListsDesc * 2)()
        d[0].n_lists, d[0].centroids = 3, None
        assert lib.slg_index_cluster_vector_field(ix._h, 0, C.addressof(d), 2) == N.ERR_INVALID  # NULL centroids
        d[0].n_lists, d[0].centroids = 65537, cents.ctypes.data
        assert lib.slg_index_cluster_vector_field(ix._h, 0, C.addressof(d), 2) == N.ERR_UNSUPPORTED
        assert rc(ix.fetch_vector_lists, 1, 0, dim)[0] == N.ERR_INVALID           # no such field
        assert rc(ix.fetch_vector_lists, 0, 2, dim)[0] == N.ERR_INVALID           # no such segment
        assert ix.fetch_vector_lists(0, 0, dim) is None
        ix.cluster_vector_field(0, [cents, N.KEEP_VECTOR_LISTS])                  # (nothing to keep: no error)
        assert rc(ix.vector_search_ivf, [0], qv, 0.0, 5, 0, 3)[0] == N.ERR_UNSUPPORTED
        assert rc(ix.vector_search_ivf, [0], qv, 0.0, 5, 257, 3)[0] == N.ERR_UNSUPPORTED
        assert rc(ix.vector_search_ivf, [0], qv, 0.0, 65, 2, 3)[0] == N.ERR_UNSUPPORTED
        assert rc(ix.vector_search_ivf, [0], qv, 0.0, 0, 2, 3)[0] == N.ERR_UNSUPPORTED
        assert rc(ix.vector_search_ivf, [3], qv, 0.0, 5, 2, 3)[0] == N.ERR_INVALID
        assert rc(ix.vector_search_ivf, [0], qv, 0.0, 5, 2, 3,
                  q_filter=np.array([0, -1], np.int32))[0] == N.ERR_INVALID       # no such filter (host form)
        cf = np.zeros(1, np.uint32)
        cnt = np.full(2, 7, np.uint32)
        assert lib.slg_vector_search_batch_ivf(ix._h, 0, 1, cf.ctypes.data, None, None, None, None, 5, 2, 3,
                                               None, None, None, None, cnt.ctypes.data, None) == 0  # nq 0
        assert (cnt == 7).all()
        got = ix.vector_search_ivf([0], qv, 0.0, 5, 3, 3)
        same(got, ix.vector_search([0], qv, 0.0, 5, 3), "after errors")
        assert int(got[4].min()) == 3
