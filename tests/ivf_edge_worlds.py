"""Worlds that sit on the edges of the IVF code (list chunks, scan carries, coarse steps, the item queue, fold passes,
unclustered chunking, build ranges), a plain host reference of the IVF call, and a mirror of the host's plan arithmetic.
numpy only: nothing here touches the device or the native library.

Exactness.  Every stored value, centroid and query component is a multiple of 1/16 of magnitude <= 1, dims are <= 64
and boosts are 1, -1 or 0.5.  A product is then a multiple of 2^-8 of magnitude <= 4 and a sum of 64 of them needs at
most 17 bits: every partial sum is exact in f32 whatever the order of the additions, so the float64 value rounded once
to f32 is the device's score, bit for bit: the dot for metric 0, -sqrt(sum of squares) for metric 1 (a correctly
rounded f32 square root of an exact f32 is the f64 one rounded once more).  check_exact() asserts this on a sample.

The reference (ivf_reference) restates the call from its documentation: the list of a row is its best centroid, ties
to the lower list; a query probes the min(nprobe, total) best (segment, list) by boosted score, then segment, then
list; the candidates are the live, unfiltered docs of the probed lists and of every unclustered segment; the result is
the best cand_size by (score desc, segment asc, doc asc), scores compared as f32::total_cmp does."""
import functools
import itertools
from types import SimpleNamespace as NS

import numpy as np

F32 = np.float32
NOVEC = 0xFFFFFFFF
N_CU = 256  # compute units of the MI355X: what the CPU tests put into the mirror of IvfAssign


# ---- exact scores ----
def scores(metric, q, v):
    """f32 [len(q), len(v)]: the score of every (query, vector) pair, computed in float64 and rounded once"""
    q64, v64 = np.asarray(q, np.float64), np.asarray(v, np.float64)
    dot = q64 @ v64.T
    if metric == 0:
        return (dot + 0.0).astype(F32)  # (the device's sum starts at +0: it is never -0)
    ss = (q64 * q64).sum(axis=1)[:, None] + (v64 * v64).sum(axis=1)[None, :] - 2.0 * dot  # exact on the grid
    return (-np.sqrt(ss)).astype(F32)


def order_key(x):
    """int64, ascending as f32::total_cmp"""
    b = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
    return b ^ ((b >> 63) & 0x7FFFFFFF)


def f32_chain(metric, q, v, order):
    """the score accumulated in f32, one dimension after another in `order`"""
    acc = F32(0.0)
    for d in order:
        t = F32(q[d]) * F32(v[d]) if metric == 0 else (F32(q[d]) - F32(v[d])) * (F32(q[d]) - F32(v[d]))
        acc = F32(acc + t)
    return acc if metric == 0 else F32(-np.sqrt(acc))


def check_exact(metric, q, v, rng, n=40):
    """on n random (query, vector) pairs: the f32 chain forwards and in a random order is the f64 value's bytes"""
    full = scores(metric, q, v)
    for _ in range(n):
        i, j = int(rng.integers(len(q))), int(rng.integers(len(v)))
        dim = q.shape[1]
        for order in (range(dim), rng.permutation(dim)):
            got = f32_chain(metric, q[i], v[j], order)
            assert got.tobytes() == full[i, j].tobytes(), (metric, i, j, got, full[i, j])


# ---- the lists ----
def assign_rows(metric, vals, cents, block=1024):
    """the list of every row: best score, ties to the lower list"""
    out = np.empty(len(vals), np.int64)
    for r0 in range(0, len(vals), block):
        out[r0:r0 + block] = np.argmax(order_key(scores(metric, vals[r0:r0 + block], cents)), axis=1)  # (first max)
    return out


def build_lists(offs, row_list, n_lists):
    """(list_begin u32 [n_lists + 1], docs u32): the docs with a vector, by (list, doc)"""
    have = np.nonzero(offs != NOVEC)[0]
    l = row_list[offs[have]]
    docs = have[np.lexsort((have, l))]
    begin = np.concatenate([[0], np.cumsum(np.bincount(l, minlength=n_lists))])
    return begin.astype(np.uint32), docs.astype(np.uint32)


def world_lists(w):
    """per segment None (unclustered) or NS(begin, docs, doc_list [n_docs] list or -1), computed once per world"""
    if w.lists is None:
        w.lists = []
        for s in w.segs:
            if s.cents is None:
                w.lists.append(None)
                continue
            rl = assign_rows(w.metric, s.vals, s.cents)
            begin, docs = build_lists(s.offs, rl, len(s.cents))
            doc_list = np.full(s.n_docs, -1, np.int64)
            have = s.offs != NOVEC
            doc_list[have] = rl[s.offs[have]]
            w.lists.append(NS(begin=begin, docs=docs, doc_list=doc_list, lens=np.diff(begin.astype(np.int64))))
    return w.lists


# ---- the call ----
def ivf_reference(w, qv, boost, q_filter, nprobe, cand, k_out):
    """w: a world (metric, segs with offs / vals / cents / deleted, own filter masks).  boost [nq] or None; q_filter
    [nq] index into w.own or -1, or None.  -> NS(seg, doc, vec [nq, k_out], count, total [nq], probes [nq, P] flat
    lists best first, list_base)"""
    metric, nq = w.metric, len(qv)
    b = np.ones(nq, F32) if boost is None else np.asarray(boost, F32).reshape(nq)
    lists = world_lists(w)
    n_lists = [0 if s.cents is None else len(s.cents) for s in w.segs]
    list_base = np.concatenate([[0], np.cumsum(n_lists)]).astype(np.int64)
    total_lists = int(list_base[-1])
    P = min(nprobe, total_lists)
    allc = np.concatenate([s.cents for s in w.segs if s.cents is not None])
    ckey = order_key(scores(metric, qv, allc) * b[:, None])
    probes = np.argsort(-ckey, axis=1, kind="stable")[:, :P]  # (stable: equal scores stay in (segment, list) order)
    probed = np.zeros((nq, total_lists), bool)
    np.put_along_axis(probed, probes, True, axis=1)
    doc_base = np.concatenate([[0], np.cumsum([s.n_docs for s in w.segs])]).astype(np.int64)
    keys, flats, oks = [], [], []
    for si, s in enumerate(w.segs):
        have = np.nonzero(s.offs != NOVEC)[0]
        sc = scores(metric, qv, s.vals)[:, s.offs[have]] * b[:, None]
        if lists[si] is None:
            ok = np.ones((nq, len(have)), bool)
        else:
            ok = probed[:, list_base[si] + lists[si].doc_list[have]]
        live = np.ones(s.n_docs, bool)
        live[np.asarray(s.deleted, np.int64)] = False
        ok &= live[have][None, :]
        if q_filter is not None:
            for q in range(nq):
                if q_filter[q] >= 0:
                    ok[q] &= w.own[int(q_filter[q])][si][have]
        keys.append(sc)
        flats.append(doc_base[si] + have)
        oks.append(ok)
    sc, flat, ok = np.concatenate(keys, axis=1), np.concatenate(flats), np.concatenate(oks, axis=1)
    out = NS(seg=np.zeros((nq, k_out), np.uint32), doc=np.zeros((nq, k_out), np.uint32), vec=np.zeros((nq, k_out), F32),
             count=np.zeros(nq, np.uint32), total=np.zeros(nq, np.uint64), probes=probes, list_base=list_base,
             top=[])
    for q in range(nq):
        idx = np.nonzero(ok[q])[0]
        idx = idx[np.lexsort((flat[idx], -order_key(sc[q, idx])))][:cand]
        out.top.append(flat[idx])  # the best cand_size, before k_out cuts them
        out.total[q] = len(idx)
        n = min(len(idx), k_out)
        out.count[q] = n
        f = flat[idx[:n]]
        sg = np.searchsorted(doc_base, f, side="right") - 1
        out.seg[q, :n] = sg
        out.doc[q, :n] = f - doc_base[sg]
        out.vec[q, :n] = F32(0.0) + sc[q, idx[:n]]  # (reported as a sum that starts at +0: -0 reads +0)
    return out


# ---- the mirror of the host's plan arithmetic: only to assert that a world reaches its edge ----
def _cdiv(a, b):
    return (a + b - 1) // b


def uncl_chunking(n_docs):
    """(chunk_docs, slots) of an unclustered segment.  Mirrors the list tables of finish_state, slg_index.hip"""
    tiles = _cdiv(n_docs, 128)
    want = min(tiles, 32)
    chunk = _cdiv(tiles, want) * 128
    return chunk, _cdiv(n_docs, chunk)


def build_ranges(n_docs, n_lists):
    """(range_docs, n_ranges).  Mirrors vs_build_lists, slg_vsearch.hip"""
    max_ranges = max(min(256, (16 << 20) // n_lists), 1)
    range_docs = _cdiv(max(4096, _cdiv(n_docs, max_ranges)), 64) * 64
    return range_docs, max(_cdiv(n_docs, range_docs), 1)


def assign_chunks(n_rows, n_lists, n_cu=N_CU):
    """(n_chunks, tiles_per_block) of IvfAssign, slg_vsearch.hip: three resident workgroups per CU"""
    n_tiles = _cdiv(n_lists, 128)
    qtiles = _cdiv(min(65536, n_rows), 64)
    n_chunks = min(max(_cdiv(3 * n_cu, qtiles), 1), n_tiles)
    tpb = _cdiv(n_tiles, n_chunks)
    return _cdiv(n_tiles, tpb), tpb


def plan(w, nq, nprobe, cand):
    """Mirrors ivf_plan and the loops of vs_lists_ivf, slg_vsearch.hip"""
    lists = world_lists(w)
    total_lists = sum(len(s.cents) for s in w.segs if s.cents is not None)
    max_len = max([int(l.lens.max()) for l in lists if l is not None and len(l.lens)] + [0])
    uncl = [uncl_chunking(s.n_docs) for s, l in zip(w.segs, lists) if l is None and s.n_docs]
    P = min(nprobe, total_lists)
    list_chunks = max(min(4, _cdiv(max_len, 1024)), 1)
    list_chunk_docs = max(_cdiv(_cdiv(max_len, list_chunks), 128) * 128, 128)
    slots_q = P * list_chunks + sum(u[1] for u in uncl)
    coarse_docs = min((16384 - P) // 128 * 128, _cdiv(total_lists, 128) * 128)
    return NS(P=P, total_lists=total_lists, max_len=max_len, list_chunks=list_chunks, list_chunk_docs=list_chunk_docs,
              uncl=uncl, uncl_slots=sum(u[1] for u in uncl), slots_q=slots_q, coarse_docs=coarse_docs,
              coarse_tiles=_cdiv(total_lists, 128), coarse_steps=_cdiv(_cdiv(total_lists, 128), coarse_docs // 128),
              fold_passes=_cdiv(slots_q * 64, 16384 - cand), fold_keys=16384 - cand,
              scan_passes=_cdiv(total_lists + len(uncl), 1024), n_ext=total_lists + len(uncl),
              qtiles=_cdiv(nq, 64))


def count_items(w, ref, pl, nq):
    """items of a call from the reference's probes: per list ceil(c_L / 64) * ceil(len_L / list_chunk_docs), and
    per unclustered segment ceil(nq / 64) * its slots"""
    lens = np.concatenate([l.lens for l in world_lists(w) if l is not None])
    c = np.bincount(ref.probes.ravel(), minlength=len(lens))
    return int((_cdiv(c, 64) * _cdiv(lens, pl.list_chunk_docs)).sum()) + _cdiv(nq, 64) * pl.uncl_slots


def slot_of(w, ref, pl, q, flat_doc):
    """the partial slot of query q that holds flat doc: (probe rank) * list_chunks + chunk, or behind them the slot
    of an unclustered segment's chunk"""
    lists = world_lists(w)
    doc_base = np.concatenate([[0], np.cumsum([s.n_docs for s in w.segs])])
    si = int(np.searchsorted(doc_base, flat_doc, side="right") - 1)
    d = int(flat_doc - doc_base[si])
    if lists[si] is None:
        slot = pl.P * pl.list_chunks
        for sj in range(si):
            if lists[sj] is None and w.segs[sj].n_docs:
                slot += uncl_chunking(w.segs[sj].n_docs)[1]
        return slot + d // uncl_chunking(w.segs[si].n_docs)[0]
    l = int(lists[si].doc_list[d])
    rank = int(np.nonzero(ref.probes[q] == ref.list_base[si] + l)[0][0])
    b = lists[si].begin
    pos = int(np.searchsorted(lists[si].docs[b[l]:b[l + 1]], d))
    return rank * pl.list_chunks + pos // pl.list_chunk_docs


def chunk_of(w, pl, flat_doc):
    """(segment, list, chunk) of a doc of a clustered segment"""
    lists = world_lists(w)
    doc_base = np.concatenate([[0], np.cumsum([s.n_docs for s in w.segs])])
    si = int(np.searchsorted(doc_base, flat_doc, side="right") - 1)
    d = int(flat_doc - doc_base[si])
    if lists[si] is None:
        return None
    l = int(lists[si].doc_list[d])
    b = lists[si].begin
    return si, l, int(np.searchsorted(lists[si].docs[b[l]:b[l + 1]], d)) // pl.list_chunk_docs


# ---- grid-valued vectors whose nearest centroid is known by construction ----
def make_cents(rng, metric, n, dim, fine=False, corners=False):
    """n distinct centroids.  metric 0: sums of three basis vectors; metric 1: points of the 1/4 lattice in
    [-0.75, 0.75]^dim (fine: of the 1/16 grid in [-1, 1]^dim, for rows that are their centroid itself; corners:
    of {-0.5, 0.5}^dim, all of one norm, so that no centroid is near every query)"""
    if metric == 0:
        combos = np.array(list(itertools.combinations(range(dim), 3)))
        assert len(combos) >= n
        pick = combos[rng.permutation(len(combos))[:n]]
        c = np.zeros((n, dim), F32)
        np.put_along_axis(c, pick, 1.0, axis=1)
        return c
    lo, hi, step = (-16, 17, 16.0) if fine else (-3, 4, 4.0)
    draw = rng.integers(lo, hi, size=(3 * n + 64, dim))
    if corners:
        draw = 4 * (draw & 1) - 2
    seen = np.unique(draw, axis=0)
    assert len(seen) >= n
    return (seen[rng.permutation(len(seen))[:n]] / step).astype(F32)


def near(rng, metric, c, noise=True):
    """one vector per row of c that is nearer c's row than any other centroid of make_cents.
    metric 0: 1 on the centroid's three dims, a multiple of 1/16 in [-0.5, 0.5] elsewhere: the own centroid scores 3,
    another at most 2.5.  metric 1: the centroid + {-1/16, 0, 1/16} per dim: in the dim where another centroid
    differs (by >= 1/4) it is at least 3/16 away, the own one at most 1/16, and the other dims add the same to both."""
    c = np.atleast_2d(c)
    if not noise:
        return c.astype(F32).copy()
    if metric == 0:
        v = (rng.integers(-8, 9, size=c.shape) / 16.0).astype(F32)
        v[c == 1.0] = 1.0
        return v
    return (c + rng.integers(-1, 2, size=c.shape) / 16.0).astype(F32)


def make_store(rng, vals, n_missing):
    """(offs, vals): every row referred to by one doc, rows out of doc order, n_missing docs without a vector"""
    n_rows = len(vals)
    n_docs = n_rows + n_missing
    have = np.ones(n_docs, bool)
    have[rng.choice(n_docs, n_missing, replace=False)] = False
    offs = np.full(n_docs, NOVEC, np.uint32)
    offs[np.nonzero(have)[0]] = rng.permutation(n_rows)
    return offs, np.ascontiguousarray(vals, F32)


def make_seg(rng, metric, cents, lens, n_missing, clustered=True, noise=True, p_deleted=0.03, extra=None):
    """a segment with lens[l] rows near cents[l] (extra: further rows as given), clustered around cents or not"""
    rows = [near(rng, metric, np.repeat(cents[l][None], n, axis=0), noise) for l, n in enumerate(lens) if n]
    if extra is not None:
        rows.append(np.asarray(extra, F32))
    offs, vals = make_store(rng, np.concatenate(rows), n_missing)
    deleted = np.nonzero(rng.random(len(offs)) < p_deleted)[0]
    return NS(n_docs=len(offs), offs=offs, vals=vals, cents=np.ascontiguousarray(cents, F32) if clustered else None,
              deleted=deleted)


def keep_live(seg, lens, lists):
    """take the docs of `lists` off the segment's tombstones (make_seg lays the rows out in list order)"""
    row0 = np.concatenate([[0], np.cumsum(lens)])
    keep = np.concatenate([np.arange(row0[l], row0[l + 1]) for l in lists])
    seg.deleted = np.array([d for d in seg.deleted if seg.offs[d] == NOVEC or seg.offs[d] not in keep], np.int64)
    return seg


def finish(name, metric, dim, segs, qv, cases, rng, p_own=(0.6, 0.1)):
    """the world: own filters (two masks), a per-query choice among them, and a mixed boost of 1, -1 and 0.5"""
    nq = len(qv)
    own = [[rng.random(s.n_docs) < p for s in segs] for p in p_own]
    own_of_query = np.where(np.arange(nq) % 4 == 1, 0, np.where(np.arange(nq) % 9 == 2, 1, -1)).astype(np.int64)
    boost = np.ones(nq, F32)
    boost[::3] = -1.0
    boost[2::5] = 0.5
    return NS(name=name, metric=metric, dim=dim, segs=segs, qv=np.ascontiguousarray(qv, F32), cases=cases, own=own,
              own_of_query=own_of_query, boost=boost, lists=None, refs={})


def reference(w, case, variant):
    """the reference of one (nprobe, cand, k_out) case of a world, computed once.  variant "filtered": tombstones and
    the per-query filters; "boost": tombstones and the mixed boost"""
    key = (case, variant)
    if key not in w.refs:
        nprobe, cand, k_out = case
        if variant == "filtered":
            w.refs[key] = ivf_reference(w, w.qv, None, w.own_of_query, nprobe, cand, k_out)
        else:
            w.refs[key] = ivf_reference(w, w.qv, w.boost, None, nprobe, cand, k_out)
    return w.refs[key]


# ---- A: list chunks ----
A_LENGTHS = {"A1": [1025, 640, 641, 1024, 1, 0], "A2": [2049, 768, 769, 1537, 1, 0], "A3": [3073, 896, 897, 2688, 2689]}
A_CHUNKS = {"A1": (2, 640), "A2": (3, 768), "A3": (4, 896)}
A_CASES = [(1, 1, 1), (2, 32, 40), (2, 33, 33), (3, 64, 64)]


@functools.lru_cache(maxsize=None)
def world_a(name, metric):
    rng = np.random.default_rng(1000 + 10 * sorted(A_LENGTHS).index(name) + metric)
    lens, dim = A_LENGTHS[name], 8
    cents = make_cents(rng, metric, len(lens), dim)
    for l, n in enumerate(lens):
        if n == 0:
            cents[l] = cents[0]  # a copy of list 0's centroid: the lower list gets the rows, this one stays empty
    seg = make_seg(rng, metric, cents, lens, 40)
    others = [l for l, n in enumerate(lens) if l and n]
    q_list = [0] * 130 + [others[i % len(others)] for i in range(3 * len(others))]
    qv = near(rng, metric, cents[q_list])
    return finish(name, metric, dim, [seg], qv, A_CASES, rng)


# ---- B: scan carries (D: the item queue, over B2's lists) ----
B_KINDS = {"B1": ([1025], False), "B2": ([2049], False), "B3": ([600, 600], False), "B4": ([1023], True),
           "B5": ([1024], True)}
B_CASES = [(1, 5, 5), (4, 33, 33), (16, 64, 64)]


def b_edge_lists(total):
    """the flat lists on both sides of every multiple of 1024, the first and the last"""
    return sorted({l for m in range(1024, total + 1, 1024) for l in (m - 1, m) if l < total} | {0, total - 1})


@functools.lru_cache(maxsize=None)
def world_b(name, metric, nq=40, cases=tuple(B_CASES), spread=False):
    """short lists (0 .. 3 docs); the lists of b_edge_lists are non-empty and have a query of their own"""
    rng = np.random.default_rng(2000 + 10 * sorted(B_KINDS).index(name) + metric)
    per_seg, with_uncl = B_KINDS[name]
    dim, total = 32, sum(per_seg)
    cents = make_cents(rng, metric, total, dim, corners=True)
    lens = rng.choice([0, 1, 1, 1, 2, 2, 2, 3], size=total)
    edge = b_edge_lists(total)
    lens[edge] = 2
    segs, c0 = [], 0
    for n in per_seg:
        segs.append(keep_live(make_seg(rng, metric, cents[c0:c0 + n], lens[c0:c0 + n], 30), lens[c0:c0 + n],
                              [l - c0 for l in edge if c0 <= l < c0 + n]))
        c0 += n
    if with_uncl:
        segs.append(make_seg(rng, metric, cents, (np.arange(total) % 5 == 0).astype(int), 10, clustered=False))
    q_cents = ([] if spread else edge) + rng.choice(total, nq, replace=False).tolist()
    qv = near(rng, metric, cents[q_cents[:nq]])
    w = finish(name, metric, dim, segs, qv, list(cases), rng)
    if not spread:   # the edge lists' own queries: no filter, boost 1, so their docs are hits in every run
        w.own_of_query[:len(edge)] = -1
        w.boost[:len(edge)] = 1.0
    return w


D_CASES = [(16, 20, 20)]


def world_d(metric):
    return world_b("B2", metric, nq=128, cases=tuple(D_CASES), spread=True)


# ---- C: coarse steps, the assignment over several chunks of centroid tiles ----
C_LISTS = 16300
C_DUPS = [(100, 16290), (5000, 9000), (4095, 4096), (16000, 16200)]  # (lower, upper): across the steps / the chunks
C_CASES = [(1, 8, 8), (2, 33, 33), (256, 64, 64)]


@functools.lru_cache(maxsize=None)
def world_c(metric):
    rng = np.random.default_rng(3000 + metric)
    dim = 4 if metric == 1 else 48
    cents = make_cents(rng, metric, C_LISTS, dim, fine=True)
    for lo, hi in C_DUPS:
        cents[hi] = cents[lo]
    lens = np.ones(C_LISTS, np.int64)
    lens[rng.choice(C_LISTS, 300, replace=False)] = 0
    lens[rng.choice(C_LISTS, 300, replace=False)] = 2
    for lo, hi in C_DUPS:
        lens[lo] = lens[hi] = 1
    lens[C_LISTS - 1] = 1
    seg = make_seg(rng, metric, cents, lens, 50, noise=metric == 0)
    q_lists = [100, 5000, 4095, 16000, 16299, 16250, 16130, 16127, 16255, 16256, 3, 8191] + \
        rng.choice(C_LISTS, 8, replace=False).tolist()
    # the first four queries are the duplicated centroids themselves: both copies tie, the lower list comes first
    qv = near(rng, metric, cents[q_lists], noise=False)
    if metric == 0:
        qv[4:] = near(rng, metric, cents[q_lists[4:]])
    w = finish("C", metric, dim, [seg], qv, C_CASES, rng)
    # a second, small store over the same centroids: one query tile of rows, so a workgroup per centroid tile
    small_lists = rng.choice(C_LISTS, 40, replace=False)
    w.small = make_seg(rng, metric, cents, np.bincount(small_lists, minlength=C_LISTS), 9, noise=metric == 0)
    return w


# ---- E: fold passes ----
E_KINDS = {"E1": (256, False, False, 256), "E2": (128, True, False, 128), "E3": (256, True, True, 256)}
E_PASSES = {"E1": 2, "E2": 3, "E3": 5}


@functools.lru_cache(maxsize=None)
def world_e(name, metric):
    """n_lists short lists; (long) the last list holds 3073 docs, four chunks, and its centroid is every query's
    last probe; (uncl) an unclustered segment behind, whose slots come last.  The own filters are per query: the
    docs of the query's first and last probe."""
    rng = np.random.default_rng(5000 + 10 * sorted(E_KINDS).index(name) + metric)
    n_lists, long_, uncl, nprobe = E_KINDS[name]
    dim, nq = 48, 9
    if metric == 0:
        # the last list's dims are nobody else's: it scores 0 against every query, as do most lists, and is the last
        c = make_cents(rng, 0, n_lists - 1, dim - 3)
        cents = np.zeros((n_lists, dim), F32)
        cents[:-1, :dim - 3] = c
        cents[-1, dim - 3:] = 1.0
    else:
        # the last list's centroid is the corner that every query, drawn from the opposite orthant, is farthest from
        cents = -np.abs(make_cents(rng, 1, n_lists, dim))
        cents[-1] = 0.75
    lens = rng.choice([1, 1, 2], size=n_lists)
    lens[-1] = 3073 if long_ else 2
    q_lists = rng.choice(n_lists - 1, nq, replace=False)
    segs = [keep_live(make_seg(rng, metric, cents, lens, 20, p_deleted=0.01), lens, q_lists)]
    qv = near(rng, metric, cents[q_lists])
    if metric == 0:
        qv[:, dim - 3:] = -0.5  # -1.5 against the last list: no list scores less
    if uncl:
        segs.append(make_seg(rng, metric, cents[q_lists], [30] * nq, 5, clustered=False))
    w = finish(name, metric, dim, segs, qv, [(nprobe, 1, 1), (nprobe, 64, 64)], rng)
    # per-query filters: the docs of the first and of the last probed list (and of the unclustered segment)
    ref = ivf_reference(w, w.qv, None, None, nprobe, 64, 64)
    l0 = world_lists(w)[0]
    w.own = []
    for q in range(nq):
        m = np.isin(l0.doc_list, [ref.probes[q, 0], ref.probes[q, -1]])
        w.own.append([m] + [np.ones(s.n_docs, bool) for s in segs[1:]])
    w.own_of_query = np.arange(nq)
    w.refs = {}
    return w


# ---- F: unclustered chunking ----
F_ORDERS = {"F1": (4096, 4097), "F2": (4097, 4096)}


@functools.lru_cache(maxsize=None)
def world_f(name, metric):
    """a small clustered segment, then two unclustered ones; the queries sit at centroid 0, whose list holds three
    docs; each unclustered segment's docs lie near the other centroids, except its last doc: centroid 0 itself"""
    rng = np.random.default_rng(6000 + 10 * sorted(F_ORDERS).index(name) + metric)
    dim, nq = 16, 9
    if metric == 0:
        cents = np.zeros((8, dim), F32)
        cents[0, :3] = 1.0
        cents[1:, 3:] = make_cents(rng, 0, 7, dim - 3)
    else:
        cents = make_cents(rng, 1, 8, dim)
    segs = [make_seg(rng, metric, cents, [3, 40, 40, 40, 40, 40, 40, 40], 10, p_deleted=0.0)]
    for n in F_ORDERS[name]:
        rows = near(rng, metric, cents[1 + rng.integers(0, 7, n - 1)])
        s = NS(n_docs=n, offs=np.full(n, NOVEC, np.uint32), vals=None, cents=None, deleted=None)
        have = np.ones(n, bool)
        have[rng.choice(n - 1, 25, replace=False)] = False
        s.vals = np.ascontiguousarray(np.concatenate([rows[:have.sum() - 1], cents[:1]]), F32)
        perm = rng.permutation(len(s.vals) - 1)
        s.offs[np.nonzero(have)[0]] = np.concatenate([perm, [len(s.vals) - 1]])  # the last doc: the last row
        s.deleted = rng.choice(n - 1, 60, replace=False)
        segs.append(s)
    qv = near(rng, metric, np.repeat(cents[:1], nq, axis=0))
    w = finish(name, metric, dim, segs, qv, [(1, 8, 8), (2, 64, 64), (8, 33, 33)], rng, p_own=(0.9, 0.8))
    for m in w.own:
        for si in (1, 2):
            m[si][-1] = True
    return w


# ---- G: build ranges ----
G1_DOCS = (4096, 4097, 8255)


@functools.lru_cache(maxsize=None)
def world_g1(metric):
    rng = np.random.default_rng(7000 + metric)
    dim, nq = 8, 9
    segs = []
    for n in G1_DOCS:
        cents = make_cents(rng, metric, 5, dim)
        n_rows = n - n // 4
        lens = np.bincount(rng.integers(0, 5, n_rows), minlength=5)
        segs.append(make_seg(rng, metric, cents, lens, n // 4))
        assert segs[-1].n_docs == n
    qv = near(rng, metric, np.concatenate([s.cents[:3] for s in segs]))
    return finish("G1", metric, dim, segs, qv, [(2, 20, 20), (15, 64, 64)], rng)


G2_DOCS = 1048577
G2_CENTS = np.array([[0.0], [10.0], [20.0], [30.0], [40.0], [50.0], [60.0], [70.0]], F32)


def world_g2():
    """dim 1, integers: (offs, vals, expected begin, expected docs).  Built on demand, never cached: 1 048 577 docs"""
    rng = np.random.default_rng(7100)
    n_missing = 1000
    vals = rng.integers(-5, 80, size=(G2_DOCS - n_missing, 1)).astype(F32)
    offs, vals = make_store(rng, vals, n_missing)
    d = np.abs(vals.astype(np.int64) - G2_CENTS[:, 0].astype(np.int64)[None, :])
    row_list = np.argmin(d, axis=1)  # numpy's nearest integer centroid, the first of two equally near
    begin, docs = build_lists(offs, row_list, len(G2_CENTS))
    return offs, vals, begin, docs


# ---- every world that is searched, by name ----
SEARCH_WORLDS = sorted(A_LENGTHS) + sorted(B_KINDS) + ["C", "D"] + sorted(E_KINDS) + sorted(F_ORDERS) + ["G1"]


def world(name, metric):
    if name in A_LENGTHS:
        return world_a(name, metric)
    if name in B_KINDS:
        return world_b(name, metric)
    if name in E_KINDS:
        return world_e(name, metric)
    if name in F_ORDERS:
        return world_f(name, metric)
    return {"C": world_c, "D": world_d, "G1": world_g1}[name](metric)
