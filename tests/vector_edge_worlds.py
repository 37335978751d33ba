"""The worlds of the vector and hybrid kernels' edge tests: plain numpy, no device (test infrastructure).

tests/test_gpu_vector_edges.py and tests/test_gpu_hybrid_edges.py run them on the device;
tests/test_vector_edge_worlds.py proves on the CPU that they hold what the device cases rest on (doc, tile,
chunk-step and slot counts, sort-space sizes, exact scores, near-tie shares) and that the vectorised references
below equal the oracle-backed ones of tests/test_gpu_vector_search.py and tests/hybrid_ref.py.

The constants restate searchlite_amd/csrc/slg_vsearch.hpp and slg_hybrid.hpp; the functions under "host rules"
restate vs_run (slg_vsearch.hip) and hy_run (slg_hybrid.hip).  A change there must make the CPU file fail.
"""
import numpy as np

from tests import hybrid_ref as R
from tests import test_gpu_vector_search as V

F32 = np.float32
NOVEC = 0xFFFFFFFF
NO_TERM = 0xFFFFFFFF

# ---- slg_vsearch.hpp ----
TILE_DOCS = 128        # kVsTileDocs
TILE_Q = 64            # kVsTileQ (16 queries per wave)
KC = 32                # kVsKc: dimensions staged per step
ROW = 36               # kVsRow
SMALL_K = 64           # kVsSmallK: cand_size up to here takes the fused top-k scan
BUF_CAP = 96           # kVsBufCap
BUF_CAP_NARROW = 40    # kVsBufCapNarrow (cand_size <= 32)
SORT_CAP = 16384       # kVsSortCap: keys the select / blend kernels sort in LDS
# ---- slg_hybrid.hpp ----
HY_THREADS = 256       # kHyThreads
HY_SPAN_MAX = 1024     # kHySpanMax
HY_MIN_GROUPS = 2048   # hy_run: a span is halved while slots / span < 2048 (down to 64)

BOOSTS = (1.0, 2.0, -1.0, -2.0)


# ------------------------------------------------------------------ host rules
def n_tiles(total_docs):
    return (total_docs + TILE_DOCS - 1) // TILE_DOCS


def scan_lds_bytes(cap):
    """vs_scan_lds_bytes(true, cap)"""
    return (TILE_DOCS + TILE_Q) * ROW * 4 + TILE_DOCS * 8 + TILE_Q * cap * 8


def topk_grid(total_docs, nq, cand, n_cu):
    """vs_run, cand_size <= kVsSmallK: (n_chunks, tiles_per_block) on a device of n_cu compute units"""
    nt, qtiles = n_tiles(total_docs), (nq + TILE_Q - 1) // TILE_Q
    cap = BUF_CAP_NARROW if cand <= SMALL_K // 2 else BUF_CAP
    per_cu = min(3, (160 << 10) // scan_lds_bytes(cap))
    target = max(n_cu, 1) * max(per_cu, 1)
    n_chunks = min(max((target + qtiles - 1) // qtiles, 1), min(nt, (SORT_CAP - SMALL_K) // SMALL_K))
    tpb = (nt + n_chunks - 1) // n_chunks
    return (nt + tpb - 1) // tpb, tpb


def min_tiles_per_block(total_docs):
    """tiles_per_block on any device: n_chunks never exceeds (kVsSortCap - kVsSmallK) / kVsSmallK = 255"""
    nt = n_tiles(total_docs)
    return (nt + 254) // 255


def store_steps(total_docs, cand):
    """vs_run, cand_size > kVsSmallK: (chunk_docs, chunk steps)"""
    chunk_docs = ((SORT_CAP - cand) // TILE_DOCS) * TILE_DOCS
    tpc = chunk_docs // TILE_DOCS
    return chunk_docs, max((n_tiles(total_docs) + tpc - 1) // tpc, 1)


def pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def blend_P(n_clauses, cand):
    """the union's sort space: in global memory when above SORT_CAP"""
    return pow2(n_clauses * cand)


def hy_span(slots):
    """hy_run: the candidate slots a workgroup of hy_gather_kernel takes; its waves = min(span, 256) / 64"""
    span = HY_SPAN_MAX
    while span > 64 and slots // span < HY_MIN_GROUPS:
        span >>= 1
    return span


def hy_threshold(span):
    """fewest slots of a launch that get this span"""
    return span * HY_MIN_GROUPS


# ------------------------------------------------------------------ vectorised vector-only reference
def _tkeys(x):
    b = np.asarray(x, F32).view(np.int32).astype(np.int64)
    return b ^ ((b >> 31) & 0x7FFFFFFF)


def similarities(metric, rows, qv):
    """metric_similarity of every row, f32 operation by operation as the oracle: the cosine sum runs left to right
    from -0.0 (NaN -> 0), L2 is -sqrt(sum (a - b)^2)"""
    qv = np.asarray(qv, F32)
    with np.errstate(all="ignore"):
        if metric == 0:
            acc = np.full(len(rows), -0.0, F32)
            for j in range(rows.shape[1]):
                acc = (acc + (rows[:, j] * qv[j]).astype(F32)).astype(F32)
            return np.where(np.isnan(acc), F32(0.0), acc).astype(F32)
        acc = np.zeros(len(rows), F32)
        for j in range(rows.shape[1]):
            d = (rows[:, j] - qv[j]).astype(F32)
            acc = (acc + (d * d).astype(F32)).astype(F32)
        return (-np.sqrt(acc)).astype(F32)


def clause_scores_fast(field, qv, bst, live_masks=None):
    """V._clause_scores without the oracle and without Python loops over docs: (score f32[n], seg[n], doc[n]) of
    every live doc with a vector, sorted by (score desc under total_cmp, segment, doc)"""
    sc, sg, dc = [], [], []
    for s, st in enumerate(field):
        if st is None:
            continue
        metric, offs, vals = st
        ok = offs != NOVEC
        if live_masks is not None:
            ok = ok & live_masks[s]
        docs = np.nonzero(ok)[0]
        if len(docs) == 0:
            continue
        with np.errstate(all="ignore"):
            sc.append((similarities(metric, vals[offs[docs]], qv) * F32(bst)).astype(F32))
        sg.append(np.full(len(docs), s, np.int64))
        dc.append(docs.astype(np.int64))
    if not sc:
        return np.zeros(0, F32), np.zeros(0, np.int64), np.zeros(0, np.int64)
    sc, sg, dc = np.concatenate(sc), np.concatenate(sg), np.concatenate(dc)
    order = np.lexsort((dc, sg, -_tkeys(sc)))
    return sc[order], sg[order], dc[order]


def _clause_dims(fields, clause_field):
    dims = [next(st[2].shape[1] for st in fields[f] if st is not None) for f in clause_field]
    return np.concatenate([[0], np.cumsum(dims)]).astype(int)


def sorted_lists(fields, clause_field, qvecs, boost, live_masks=None):
    """[q][c] = clause_scores_fast of the whole field: cut to any cand_size by reference_from_lists"""
    offs = _clause_dims(fields, clause_field)
    return [[clause_scores_fast(fields[f], qvecs[q, offs[c]:offs[c + 1]], boost[q, c], live_masks)
             for c, f in enumerate(clause_field)] for q in range(len(qvecs))]


def list_gap(lists_q, boost_q, cand):
    """V.boundary_gap of one query from its sorted lists"""
    gap = np.inf
    for (sc, _, _), b in zip(lists_q, boost_q):
        if b != 0 and len(sc) > cand:
            gap = min(gap, abs(float(sc[cand - 1]) - float(sc[cand])))
    return gap


def reference_from_lists(lists, metrics, clause_field, alpha, cand, k_out):
    """V.reference from sorted_lists: the union and the blend are V.blend_rows"""
    out = []
    for q, lq in enumerate(lists):
        maps = [{(int(s), int(d)): v for v, s, d in zip(sc[:cand], sg[:cand], dc[:cand])} for sc, sg, dc in lq]
        rows, total = V.blend_rows(maps, metrics, clause_field, alpha[q], k_out)
        out.append((rows, total, maps))
    return out


def queries_with_gap(rng, fields, clause_field, dims, metric_of, nq, boost, cands, live_masks=None, tail=None):
    """V._queries over sorted lists: queries whose gap at every cand_size of `cands` is >= 1e-4 (redrawn otherwise).
    tail: (n, value per metric) overwrites the last n components of every clause vector"""
    qs = []
    while len(qs) < nq:
        parts = []
        for c, d in enumerate(dims):
            p = V._unit(rng, 1, d)[0] if metric_of[c] == 0 else (rng.standard_normal(d) / np.sqrt(d)).astype(F32)
            if tail is not None:
                p[d - tail[0]:] = tail[1][metric_of[c]]
            parts.append(p)
        qv = np.concatenate(parts).astype(F32)[None, :]
        lq = sorted_lists(fields, clause_field, qv, boost[len(qs):len(qs) + 1], live_masks)[0]
        if all(list_gap(lq, boost[len(qs)], cand) >= 1e-4 for cand in cands):
            qs.append(qv[0])
    return np.stack(qs).astype(F32)


# ------------------------------------------------------------------ exact-score worlds
class VecWorld:
    """stores[s] = (metric, offsets, values) or None; dels[s] = deleted docs; live_masks[s] = not deleted"""

    def __init__(self, n_docs, stores, dels=None):
        self.n_docs, self.stores, self.dels = list(n_docs), stores, dict(dels or {})
        self.total = sum(n_docs)
        self.live_masks = []
        for s, n in enumerate(n_docs):
            m = np.ones(n, bool)
            m[list(self.dels.get(s, ()))] = False
            self.live_masks.append(m)

    def live(self, q, s, d):
        return bool(self.live_masks[s][d])

    def n_live_vectors(self):
        return sum(int(((st[1] != NOVEC) & self.live_masks[s]).sum()) for s, st in enumerate(self.stores) if st)

    def segs(self):
        out = []
        for s, (n, st) in enumerate(zip(self.n_docs, self.stores)):
            sg = V._seg(n) if st is None else V._seg(n, st[1], st[2], metric=st[0])
            if self.dels.get(s):
                sg.set_deleted(sorted(self.dels[s]))
            out.append(sg)
        return out


def exact_world(n_docs, dim, order, seed, p_missing=0.1, dels=None, no_field=(), zeros=()):
    """Cosine stores whose rows are (v, 0, .., 0): against a query (x, 0, .., 0) a doc scores round(v * x) in one
    rounding, on the matrix cores' fma chain as in the oracle's sum, and a boost of +-1 / +-2 keeps it exact.
    v = m / 65536 with m an integer below 2^17, distinct per doc, laid over the flat docs (segment, doc) by `order`:
      "asc"  m = flat + 1: every doc beats all before it      "desc" m = total - flat: nothing after the first does
      "perm" m = a random permutation of 1 .. total           "tied" v = 0.5 everywhere: (segment, doc) alone decides
    About p_missing of the docs have no vector (never the first or the last doc); the rows are stored out of doc
    order; segments in no_field have no store; flats in `zeros` hold the zero vector."""
    rng = np.random.default_rng(seed)
    total = sum(n_docs)
    assert total < (1 << 17)
    flat = np.arange(total)
    m = {"asc": flat + 1, "desc": total - flat, "perm": rng.permutation(total) + 1,
         "tied": np.full(total, 32768)}[order]
    v = (m / 65536.0).astype(F32)
    v[list(zeros)] = 0.0
    have = rng.random(total) >= p_missing
    have[0] = have[-1] = True
    have[list(zeros)] = True
    stores, base = [], 0
    for s, n in enumerate(n_docs):
        if s in no_field:
            stores.append(None)
            base += n
            continue
        docs = np.nonzero(have[base:base + n])[0]
        perm = rng.permutation(len(docs))
        offs = np.full(n, NOVEC, np.uint32)
        offs[docs] = perm
        vals = np.zeros((max(len(docs), 1), dim), F32)
        vals[perm, 0] = v[base + docs]
        stores.append((0, offs, vals))
        base += n
    return VecWorld(n_docs, stores, dels)


def exact_queries(nq, dim, boosts=BOOSTS):
    """pairwise distinct queries (1 + q / 256, 0, .., 0) and a nonzero boost per query, cycling through `boosts`"""
    qv = np.zeros((nq, dim), F32)
    qv[:, 0] = (1.0 + np.arange(nq) / 256.0).astype(F32)
    return qv, np.array([boosts[q % len(boosts)] for q in range(nq)], F32)[:, None]


def closed_form_scores(W, qv, boost, q):
    """{(seg, doc): score} of query q over an exact world, from the first components alone"""
    out = {}
    for s, st in enumerate(W.stores):
        if st is None:
            continue
        _, offs, vals = st
        for d in np.nonzero((offs != NOVEC) & W.live_masks[s])[0]:
            out[(s, int(d))] = F32(F32(vals[offs[d], 0] * qv[q, 0]) * boost[q, 0])
    return out


# the big world of test_multi_tile_blocks and test_store_path_steps
BIG_DOCS = (50_000, 48_049)       # 3 * 32 640 + 129: 767 tiles, the last of one doc; the boundary 80 docs into a tile
BIG_DELS = {0: {0, 1, 5, 31_999, 49_999}, 1: {0, 77, 48_000, 48_047}}
BIG_DIM = 4
BIG_ORDERS = ("asc", "desc", "tied")
_cache = {}


def big_world(order):
    if ("big", order) not in _cache:
        _cache["big", order] = exact_world(BIG_DOCS, BIG_DIM, order, seed=4100, dels=BIG_DELS)
    return _cache["big", order]


def big_random_world():
    """the big world's layout with random unit vectors"""
    if "bigrand" not in _cache:
        W = exact_world(BIG_DOCS, BIG_DIM, "tied", seed=4100, dels=BIG_DELS)
        rng = np.random.default_rng(4101)
        W.stores = [(0, offs, V._unit(rng, len(vals), BIG_DIM)) for _, offs, vals in W.stores]
        _cache["bigrand"] = W
    return _cache["bigrand"]


def big_lists(order, nq=3):
    """the big world's queries (boosts 1, 2, -1) and every query's whole sorted list, computed once"""
    if ("lists", order) not in _cache:
        W = big_world(order)
        qv, boost = exact_queries(nq, BIG_DIM, boosts=(1.0, 2.0, -1.0))
        _cache["lists", order] = (qv, boost, sorted_lists([W.stores], [0], qv, boost, W.live_masks))
    return _cache["lists", order]


def big_random_lists(cands=(32, 64), nq=3):
    if "randlists" not in _cache:
        W = big_random_world()
        boost = np.ones((nq, 1), F32)
        qv = queries_with_gap(np.random.default_rng(4102), [W.stores], [0], [BIG_DIM], [0], nq, boost, cands,
                              W.live_masks)
        _cache["randlists"] = (qv, boost, sorted_lists([W.stores], [0], qv, boost, W.live_masks))
    return _cache["randlists"]


# test_doc_tile_edges
DOC_TILE_TOTALS = (1, 127, 128, 129, 256, 257)
THREE_SEGS = (64, 64, 1)          # boundaries at flats 64, 128, 129; the middle segment has no vector field


def doc_tile_world(name):
    if name == "3seg":
        return exact_world(THREE_SEGS, 8, "perm", seed=4300, no_field=(1,), dels={0: {3, 40}})
    return exact_world((name,), 8, "perm", seed=4300 + name, dels={0: {n for n in (2, 100) if n < name}})


QUERY_TILE_NQS = (15, 16, 17, 63, 64, 65, 129)


def query_tile_world():
    return exact_world((170, 130), 8, "perm", seed=4200, dels={0: {4, 9, 169}, 1: {0, 64}})


def signed_zero_world():
    """two fields over 2 x 60 docs.  Field 0: exact "perm" rows, ten of them the zero vector (score +0.0, -0.0 under
    a boost of -1).  Field 1: the zero vector everywhere (every doc scores +0.0 under a boost of +1)."""
    zeros = (3, 17, 18, 59, 60, 61, 90, 100, 118, 119)
    A = exact_world((60, 60), 8, "perm", seed=4400, dels={0: {7}, 1: {5}}, zeros=zeros)
    B = exact_world((60, 60), 8, "perm", seed=4401, dels={0: {7}, 1: {5}}, zeros=range(120))
    return A, B, zeros


NAN_FLATS = (2, 50, 79, 81, 140)
ZERO_FLATS = (1, 3, 60, 80, 82, 159)


def nan_world():
    """2 x 80 docs, exact "perm" rows; NAN_FLATS hold inf in component 3 (the query has 0.0 there: the sum is NaN and
    the score 0.0 * boost), ZERO_FLATS the zero vector (real zeros).  Boost -1 puts every zero above the rest."""
    W = exact_world((80, 80), 8, "perm", seed=4500, dels={1: {11}}, zeros=NAN_FLATS + ZERO_FLATS)
    base = 0
    for s, (_, offs, vals) in enumerate(W.stores):
        for f in NAN_FLATS:
            if base <= f < base + W.n_docs[s]:
                vals[offs[f - base], 3] = np.inf
        base += W.n_docs[s]
    return W




# test_dim_steps: dims on both sides of the 32-dimension staging step; L2 at dims that are no multiple of 4
DIM_STEPS = {0: (31, 32, 33, 36, 63, 64, 65), 1: (5, 31, 33, 36)}
# The last component of every row and query: a dropped or doubled tail dimension moves a score by 0.25 (cosine:
# 0.5 * 0.5) or turns a sum of about 2 + 1 into 2 (L2: (0.5 - -0.5)^2 = 1), 1e4 x TOL and more.  A value like
# 100 would not do: scores near 1e4 are 9.8e-4 apart in f32, so the two summation orders (the matrix cores' and
# left to right) could differ by a hundred times TOL = 1e-5 with both sides right.  With these values the
# scores stay below 2 in magnitude (f32 spacing 2.4e-7), as in test_dims_cosine.
DIM_TAIL = (1, {0: F32(0.5), 1: F32(0.5)})
DIM_ROW_TAIL = {0: F32(0.5), 1: F32(-0.5)}


def dim_world(dim, metric):
    """three segments (the middle one without the field), 20 % of the docs without a vector, tombstones"""
    rng = np.random.default_rng(4600 + 100 * metric + dim)
    n_docs = (300, 40, 257)
    stores = []
    for s, n in enumerate(n_docs):
        if s == 1:
            stores.append(None)
            continue
        vals = None if metric == 0 else (rng.standard_normal((n, dim)) / np.sqrt(dim)).astype(F32)
        m, offs, vals = V._store(rng, n, dim, metric, values=vals)
        vals = vals.copy()
        vals[:, dim - 1] = DIM_ROW_TAIL[metric]
        stores.append((m, offs, vals))
    W = VecWorld(n_docs, stores, {0: {3, 7, 100, 299}, 2: set(range(0, 257, 5))})
    nq = 4
    boost = np.ones((nq, 1), F32)
    qv = queries_with_gap(rng, [stores], [0], [dim], [metric], nq, boost, (20, 70), W.live_masks, tail=DIM_TAIL)
    return W, qv, boost


# test_union_in_global_memory: (n_clauses, cand_size); two fields of about 10 000 docs
UNION_CASES = ((2, 9000), (3, 5500))
UNION_DOCS = (6000, 5000)


def union_world(nc, cand):
    key = ("union", nc, cand)
    if key not in _cache:
        rng = np.random.default_rng(4700 + nc)
        fields = [[V._store(rng, n, 8, 0, p_missing=0.08) for n in UNION_DOCS] for _ in range(2)]
        W = VecWorld(UNION_DOCS, fields[0], {0: {1, 2, 3}, 1: {4999}})
        clause_field = [c % 2 for c in range(nc)]
        nq = 3
        boost = np.full((nq, nc), 40.0, F32)
        qv = queries_with_gap(rng, fields, clause_field, [8] * nc, [0] * nc, nq, boost, (cand,), W.live_masks)
        alpha = np.zeros((nq, nc), F32)
        alpha[1] = 0.3
        _cache[key] = (W, fields, clause_field, qv, alpha, boost,
                       sorted_lists(fields, clause_field, qv, boost, W.live_masks))
    return _cache[key]


# ------------------------------------------------------------------ hybrid: row chunks
CHUNK_DIMS = (252, 256, 260, 300, 512, 516, 764, 768, 772)
CHUNK_CASES = tuple((d, m) for d in CHUNK_DIMS for m in (0, 1))
CHUNK_DOCS = (170, 130)
CHUNK_VOCAB = 30
CHUNK_NQ, CHUNK_CAND, CHUNK_K, CHUNK_ALPHA = 8, 20, 11, 0.4
# Last four components of rows / queries: cosine 0.25 * 0.25 each (a dropped 4-float tail loses 0.25 of a score
# below 1.3 in magnitude); L2 (0.25 - -0.25)^2 each, 1.0 on a sum of about 2.  L2 rows and queries are
# standard normal / sqrt(dim), so distances are near 1.4 and the order of a 772-term f32 sum moves them by far
# less than TOL = 1e-5 (unit-variance components would give sums near 1500, where it does not).
CHUNK_Q_TAIL = F32(0.25)
CHUNK_ROW_TAIL = {0: F32(0.25), 1: F32(-0.25)}
# crafted lists: (segment, docs with a vector, docs without): one 64-candidate batch each
CHUNK_LISTS = {"m7": (0, 7, 3), "m1": (0, 1, 5), "m61": (1, 61, 3)}


class ChunkWorld:
    pass


def chunk_world():
    """About 300 docs in two segments with text, 30 % of the docs without a vector (the same docs in every field),
    three crafted lists (CHUNK_LISTS), tombstones.  Field 0 (the segment descriptors') is a 4-dimension stand-in;
    the field of case i is i + 1, added with add_vector_field."""
    if "chunk" in _cache:
        return _cache["chunk"]
    from tests.util import random_segment, _append_lists
    rng = np.random.default_rng(4800)
    W = ChunkWorld()
    W.have = [rng.random(n) >= 0.3 for n in CHUNK_DOCS]
    W.dels = {0: {2, 50}, 1: {7}}
    segs = [random_segment(rng, n, CHUNK_VOCAB, 6) for n in CHUNK_DOCS]
    W.lists, extra = {}, [[], []]
    for name, (s, with_vec, without) in CHUNK_LISTS.items():
        live = np.array([d not in W.dels.get(s, ()) for d in range(CHUNK_DOCS[s])])
        docs = np.sort(np.concatenate([rng.choice(np.nonzero(W.have[s] & live)[0], with_vec, replace=False),
                                       rng.choice(np.nonzero(~W.have[s] & live)[0], without, replace=False)]))
        W.lists[name] = (s, CHUNK_VOCAB + len(extra[s]), docs.astype(np.uint32))
        extra[s].append((docs.astype(np.uint32), np.ones(len(docs), np.uint32)))
    segs = [_append_lists(sg, extra[s]) for s, sg in enumerate(segs)]
    W.rows = [int(h.sum()) for h in W.have]
    W.offsets = []
    for s, n in enumerate(CHUNK_DOCS):
        offs = np.full(n, NOVEC, np.uint32)
        offs[np.nonzero(W.have[s])[0]] = rng.permutation(W.rows[s])
        W.offsets.append(offs)
    st0 = [(0, W.offsets[s], V._unit(rng, W.rows[s], 4)) for s in range(2)]
    for s, (sg, st) in enumerate(zip(segs, st0)):
        sg.vec_dim, sg.vec_metric, sg.vec_offsets, sg.vec_values = 4, 0, st[1], st[2]
        sg.set_deleted(sorted(W.dels[s]))
    W.segs, W.field0 = segs, st0
    # queries 0..2: the crafted lists alone; 3..7: three random words
    from tests.util import random_queries
    offs, terms, w = random_queries(rng, CHUNK_NQ - 3, 3, CHUNK_VOCAB, n_segs=2)
    crafted = np.full((3, 2), NO_TERM, np.uint32)
    for i, name in enumerate(CHUNK_LISTS):
        s, t, _ = W.lists[name]
        crafted[i, s] = t
    W.qs = (np.concatenate([np.arange(3, dtype=np.uint32), 3 + offs]).astype(np.uint32),
            np.concatenate([crafted, terms]).astype(np.uint32), np.ones(3 + len(w), F32))
    _cache["chunk"] = W
    return W


GAP = 4e-5    # test_gpu_hybrid.GAP: a query whose reference gap is below it is left out of the order check


def chunk_field(oracle, dim, metric):
    """-> (stores per segment, qvecs [CHUNK_NQ, dim]) of one case.  A query whose boundary gap in the reference is
    below GAP is redrawn (as V._queries does), so no query of these cases is left out of the order check."""
    key = ("chunkfield", dim, metric)
    if key in _cache:
        return _cache[key]
    W = chunk_world()
    rng = np.random.default_rng(4900 + 10 * dim + metric)

    def draw(n, tail):
        v = V._unit(rng, n, dim) if metric == 0 else (rng.standard_normal((n, dim)) / np.sqrt(dim)).astype(F32)
        v[:, dim - 4:] = tail
        return v

    stores = [(metric, W.offsets[s], draw(W.rows[s], CHUNK_ROW_TAIL[metric])) for s in range(2)]
    qv = draw(CHUNK_NQ, CHUNK_Q_TAIL)
    while True:
        want = R.reference(oracle, W.segs, [stores], [0], *W.qs, CHUNK_K, qv, CHUNK_ALPHA, None, CHUNK_CAND, CHUNK_K)
        bad = [q for q, w in enumerate(want) if w["gap"] < GAP]
        if not bad:
            break
        qv[bad] = draw(len(bad), CHUNK_Q_TAIL)
    _cache[key] = (stores, qv)
    return _cache[key]


# ------------------------------------------------------------------ hybrid: multi-wave workgroups
WAVE_DOCS = (23_000, 18_000)
WAVE_VOCAB = 20
WAVE_DIM = 8
WAVE_CASES = {128: 9, 256: 18, 1024: 70}    # span -> queries
WAVE_CAND, WAVE_K = 20, 11


def wave_world():
    """test_gpu_hybrid._all_docs_world over two segments, every 97th doc of segment 0 and every 89th of segment 1
    deleted"""
    if "wave" not in _cache:
        from tests.test_gpu_hybrid import _all_docs_world
        rng = np.random.default_rng(5000)
        segs, st0 = _all_docs_world(rng, list(WAVE_DOCS), WAVE_VOCAB, WAVE_DIM)
        dels = {0: set(range(5, WAVE_DOCS[0], 97)), 1: set(range(0, WAVE_DOCS[1], 89))}
        for s, sg in enumerate(segs):
            sg.set_deleted(sorted(dels[s]))
        W = VecWorld(WAVE_DOCS, st0, dels)
        W.text_segs = segs
        _cache["wave"] = W
    return _cache["wave"]


WAVE_ALPHA = 0.5


def wave_queries(oracle, span):
    """nq queries over the all-docs term (id WAVE_VOCAB); two of three add a word, so the regions differ in length;
    the middle query has no term at all.  Distinct vectors and boosts; a query whose boundary gap in the reference
    is below GAP is redrawn, so every query's order, count and total are checked.
    -> (offs, terms, w), qvecs, boost, the reference"""
    if ("waveq", span) in _cache:
        return _cache["waveq", span]
    W = wave_world()
    nq = WAVE_CASES[span]
    rng = np.random.default_rng(5100 + span)
    offs, terms = [0], []
    for q in range(nq):
        if q == nq // 2:
            terms.append([NO_TERM, NO_TERM])
        else:
            terms.append([WAVE_VOCAB, WAVE_VOCAB])
            if q % 3:
                t = int(rng.integers(0, WAVE_VOCAB))
                terms.append([t, t])
        offs.append(len(terms))
    qs = (np.array(offs, np.uint32), np.array(terms, np.uint32), np.ones(len(terms), F32))
    qv = V._unit(rng, nq, WAVE_DIM)
    boost = (1.0 + rng.random((nq, 1)) * 2.0).astype(F32)
    want, todo = [None] * nq, set(range(nq))
    while todo:
        part = hybrid_reference_all_docs(oracle, W, qs, WAVE_K, qv, WAVE_ALPHA, boost, WAVE_CAND, WAVE_K, only=todo)
        for q in sorted(todo):
            want[q] = part[q]
            if part[q]["gap"] >= GAP:
                todo.discard(q)
            else:
                qv[q] = V._unit(rng, 1, WAVE_DIM)[0]
    _cache["waveq", span] = (qs, qv, boost, want)
    return _cache["waveq", span]


def query_slots(segs, offs, terms):
    """candidate slots of each query: the lengths of its posting lists over every segment (hybrid
    pipeline step 3: a sub-query's region is as long as its posting lists)"""
    out = np.zeros(len(offs) - 1, np.int64)
    for q in range(len(out)):
        for i in range(int(offs[q]), int(offs[q + 1])):
            for s, sg in enumerate(segs):
                t = int(terms[i, s])
                if t != NO_TERM and t + 1 < len(sg.term_offsets):
                    out[q] += int(sg.term_offsets[t + 1]) - int(sg.term_offsets[t])
    return out


def queries_at_slots(slots, at):
    """the queries whose regions hold the candidate slots `at`"""
    ends = np.cumsum(slots)
    return sorted({int(np.searchsorted(ends, a, side="right")) for a in at if a < ends[-1]})


def hybrid_reference_all_docs(oracle, W, qs, k, qvecs, alpha, boost, cand, k_out, only=None):
    """R.reference for queries over the all-docs term of wave_world (or with no term): the matched set of a query
    is every live doc (or nothing), so the clause list is clause_scores_fast over the live docs, and the BM25
    hits are the oracle's top k.  only: the queries to compute (others None)."""
    offs, terms, w = qs
    nq = len(offs) - 1
    alpha = np.broadcast_to(np.asarray(alpha, F32), (nq, 1))
    hits = oracle.search_batch(W.text_segs, offs, terms, w, k)
    doc, seg, score, count = hits[:4]
    out = []
    for q in range(nq):
        if only is not None and q not in only:
            out.append(None)
            continue
        has_all = any(int(terms[i, 0]) == WAVE_VOCAB for i in range(int(offs[q]), int(offs[q + 1])))
        assert has_all or offs[q + 1] - offs[q] == 1 and int(terms[offs[q], 0]) == NO_TERM
        bm = [(int(seg[q, i]), int(doc[q, i]), F32(score[q, i])) for i in range(int(count[q]))]
        if has_all:
            sc, sg, dc = clause_scores_fast(W.stores, qvecs[q], boost[q, 0], W.live_masks)
        else:
            sc, sg, dc = np.zeros(0, F32), np.zeros(0, np.int64), np.zeros(0, np.int64)
        m = {(int(s), int(d)): F32(v) for v, s, d in zip(sc[:cand], sg[:cand], dc[:cand])}
        gap, near = np.inf, set()
        if len(sc) > cand:
            g = abs(float(sc[cand - 1]) - float(sc[cand]))
            gap = g if g > 0 else np.inf
            lo, hi = float(sc[cand]), float(sc[cand - 1])
            f = sc.astype(np.float64)
            sel = (f >= lo - R.NEAR) & (f <= hi + R.NEAR)
            near = {(int(s), int(d)) for s, d in zip(sg[sel], dc[sel])}
        rows, total, g = R.merge_vector_hits(bm, [m], alpha[q], [0], k_out)
        every, _, _ = R.merge_vector_hits(bm, [m], alpha[q], [0], total)
        near |= R.boundary_keys([(r[2], r[0], r[1]) for r in every], k_out)
        out.append(dict(rows=rows, total=total, bm25=bm, gap=min(gap, g if g > 0 else np.inf), maps=[m], near=near))
    return out
