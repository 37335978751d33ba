"""The worlds of the two-pass vector search's edge tests: plain numpy, no device (test infrastructure).

tests/test_gpu_vector_approx_edges.py runs them on the device; tests/test_vector_approx_edge_worlds.py proves on
the CPU that each reaches the path of vs_scan_bf16_kernel (slg_vsearch_approx.hpp) its case names and that a named
defect of the first pass would move its output.

The constants and the functions under "host rules" restate slg_vsearch_approx.hpp and vs_plan(..., bf16 = true) of
slg_vsearch.hip; what the bf16 plan shares with the exact one comes from tests/vector_edge_worlds.py (E).

bf16-exact worlds.  Every stored and every query component is a bf16 value (the low 16 bits of the f32 are zero),
and every product and every partial sum of a score is an integer multiple of one power of two below 2^24 times it,
so f32 adds them without rounding in any order: the first pass over the bf16 copy computes the exact scan's score,
for L2 too (|x|^2, |q|^2, 2 x.q and |x|^2 + |q|^2 - 2 x.q are such sums, and sqrtf is monotone and keeps distinct
integers below 2^20 distinct: sqrt(n + 1) - sqrt(n) > 2^-12 there, sixteen f32 steps at 1024).  Then the two-pass
call must return the exact call's bytes at any refine >= cand.

General data: the model of the first pass and its error bound (first_pass_model).
  cosine  the device rounds x_i and q_i to bf16 (nearest even), forms the products p_i = bf16(x_i) bf16(q_i), which
          are exact in f32 (8 x 8 significant bits), and adds them in f32 on the matrix cores, in an order and with
          a rounding this project does not rely on: n = dim_pad additions (the padding adds zeros), each with a
          relative error of at most u = 2^-23 (twice the unit roundoff of round-to-nearest, which covers truncation
          as well).  By the standard bound for a sum in any order, |fl(sum p_i) - sum p_i| <= g A with
          A = sum |p_i| and g = n u / (1 - n u).  The multiply by the boost adds one rounding:
              delta = |boost| (g A + u (|s~| + g A)),   s~ = sum p_i in float64.
  L2      D~ = nrm + qn - 2 s~ from the stored f32 norm of the f32 row and the f32 norm of the f32 query, both
          summed left to right in f32 (bit for bit what the device holds; the build has -ffp-contract=off).  The
          device computes fl(fl(nrm + qn) - fl(2 s)): e_D = 2 g A + u (nrm + qn) + u (|D~| + 2 g A + u (nrm + qn)).
          max(., 0) is 1-Lipschitz, |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= min(sqrt |a - b|,
          |a - b| / sqrt max(D~, 0)), and sqrtf and the multiply by the boost add one rounding each:
              delta = |boost| (e_s + 2 u (sqrt max(D~, 0) + e_s)),   e_s = min(sqrt e_D, e_D / sqrt max(D~, 0)).
  With T the model's best R docs and t its R-th score: a doc d of T that is not returned has lost its place to a doc
  e outside T, so m_d - delta_d <= dev(d) <= dev(e) <= t + delta_e; a returned doc d outside T has taken the place
  of a doc e of T, so m_d + delta_d >= t - delta_e.  Which e is not known, so the band of a doc is its own delta
  plus the largest delta of the query: |m_d - t| <= delta_d + max_e delta_e is free, everything else is asserted.
"""
import numpy as np

from tests import test_gpu_vector_search as V
from tests import vector_edge_worlds as E

F32 = np.float32
F64 = np.float64
NOVEC = E.NOVEC

# ---- slg_vsearch_approx.hpp / vs_plan(bf16) ----
KC = 64                # kVaKc: bf16 dimensions staged per step, two MFMA k-steps of 32
BY_VGPRS = 2           # resident workgroups per CU the registers of vs_scan_bf16_kernel allow
U = 2.0 ** -23         # the relative error allowed per f32 addition of the first pass


# ------------------------------------------------------------------ host rules
def dim_pad(dim):
    return (dim + KC - 1) // KC * KC


def stages(dim):
    """staging steps of a tile: the prefetch chain is this deep"""
    return dim_pad(dim) // KC


def scan_lds_bytes(cap):
    """va_scan_lds_bytes(true, cap): the exact scan's + the 128 norms"""
    return E.scan_lds_bytes(cap) + E.TILE_DOCS * 4


def topk_grid(total_docs, nq, refine, n_cu):
    """vs_plan(bf16), refine <= kVsSmallK: (n_chunks, tiles_per_block) on a device of n_cu compute units"""
    nt, qtiles = E.n_tiles(total_docs), (nq + E.TILE_Q - 1) // E.TILE_Q
    cap = E.BUF_CAP_NARROW if refine <= E.SMALL_K // 2 else E.BUF_CAP
    per_cu = min(BY_VGPRS, (160 << 10) // scan_lds_bytes(cap))
    target = max(n_cu, 1) * max(per_cu, 1)
    n_chunks = min(max((target + qtiles - 1) // qtiles, 1), min(nt, (E.SORT_CAP - E.SMALL_K) // E.SMALL_K))
    tpb = (nt + n_chunks - 1) // n_chunks
    return (nt + tpb - 1) // tpb, tpb


def qvec4(q_floats, coff, ptr=0):
    """vs_qvec4: are 16-byte loads of a clause's query vectors aligned?"""
    return int(q_floats % 4 == 0 and coff % 4 == 0 and ptr % 16 == 0)


def is_bf16(a):
    return not np.any(np.ascontiguousarray(a, F32).view(np.uint32) & np.uint32(0xFFFF))


def bf16_round(a):
    """f32 -> the nearest bf16 value (ties to even), as f32; finite values only"""
    b = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(F32)


def norms_l2r(vals):
    """left-to-right f32 sum of squares of each row (vs_quantize_kernel's norm; the scan's |q|^2)"""
    out = np.zeros(len(vals), F32)
    with np.errstate(all="ignore"):
        for k in range(vals.shape[1]):
            out = (out + (vals[:, k] * vals[:, k]).astype(F32)).astype(F32)
    return out


# ------------------------------------------------------------------ the flat view and the first-pass model
def flat_view(W):
    """(rows f32 [total, dim] (zero where a doc has no vector), ok [total]: live, with a vector) over the flat docs"""
    dim = next(st[2].shape[1] for st in W.stores if st is not None)
    rows, ok = np.zeros((W.total, dim), F32), np.zeros(W.total, bool)
    base = 0
    for s, (n, st) in enumerate(zip(W.n_docs, W.stores)):
        if st is not None:
            docs = np.nonzero(st[1] != NOVEC)[0]
            rows[base + docs] = st[2][st[1][docs]]
            ok[base + docs] = W.live_masks[s][docs]
        base += n
    return rows, ok


def flat_keys(W, flats):
    """[(segment, doc)] of flat docs"""
    base = np.concatenate([[0], np.cumsum(W.n_docs)])
    seg = np.searchsorted(base, flats, side="right") - 1
    return [(int(s), int(f - base[s])) for s, f in zip(seg, flats)]


MUTATIONS = ("drop_last_dim", "drop_second_kstep", "prev_tile_rows", "tile_begin_zero", "neighbour_query",
             "unmasked_lanes", "drop_row_127", "keep_nan")


def first_pass_top(view, metric, qv, boost, R, mut=None, tpb=1, chunk_docs=None):
    """The first pass over a bf16-exact world in float64 (exact there): per query the flat docs of its best R keys,
    best first, ties by flat doc.  mut names a defect of vs_scan_bf16_kernel:
      drop_last_dim      the dot product stops one dimension early (norms are the stored ones)
      drop_second_kstep  the second 32-wide MFMA k-step of every 64-dimension stage is left out
      prev_tile_rows     from the second tile of a workgroup on (tiles_per_block = tpb), the last stage's rows are
                         those of the tile before: the prefetch chain was started from the old drow
      tile_begin_zero    the store form indexes its output by base + i: only the first chunk step (chunk_docs docs)
                         lands inside a query's row
      neighbour_query    query row r is staged from row r ^ 1
      unmasked_lanes     the lanes past nq of the last query tile run with a zero query and boost 1, and their lists
                         land on the rows of queries q' - nq, q' - 2 nq, ..: the nearest in-bounds stand-in for a
                         write past the key buffer
      drop_row_127       the last row of every doc tile is not scored
      keep_nan           a NaN dot product is not mapped to 0 (its key is above every number's)"""
    rows, ok = view
    total, dim = rows.shape
    nq = len(qv)
    flat = np.arange(total)
    X, Q = rows.astype(F64), np.asarray(qv, F32).astype(F64)
    b = np.asarray(boost, F32).astype(F64).reshape(nq, -1)[:, 0]
    with np.errstate(all="ignore"):
        nrm, qn = (X * X).sum(1), (Q * Q).sum(1)
    Xd, Qd, valid = X, Q, ok.copy()
    if mut == "drop_last_dim":
        Xd = X.copy()
        Xd[:, -1] = 0
    elif mut == "drop_second_kstep":
        Xd = X.copy()
        Xd[:, (np.arange(dim) % KC) >= KC // 2] = 0
    elif mut == "prev_tile_rows":
        stale = (flat // E.TILE_DOCS) % tpb != 0
        Xd = X.copy()
        last = np.arange(dim) >= dim_pad(dim) - KC
        src = np.maximum(flat - E.TILE_DOCS, 0)
        Xd[np.ix_(stale, last)] = X[np.ix_(src[stale], last)]
    elif mut == "tile_begin_zero":
        valid &= flat < chunk_docs
    elif mut == "neighbour_query":
        idx = np.arange(nq) ^ 1
        idx[idx >= nq] = nq - 1
        Qd = Q[idx]
    elif mut == "drop_row_127":
        valid &= flat % E.TILE_DOCS != E.TILE_DOCS - 1
    cand = np.nonzero(valid)[0]

    def lists(Qd, qn, b):
        out = []
        with np.errstate(all="ignore"):
            # (a product 0 * inf is NaN, as on the device; numpy's matmul would spread it over the row)
            S = np.stack([(Xd[cand] * q[None, :]).sum(1) for q in Qd], axis=1)
        for q in range(len(Qd)):
            s = S[:, q]
            if metric == 0:
                s = np.where(np.isnan(s), np.inf if mut == "keep_nan" else 0.0, s)
            else:
                s = -np.sqrt(np.maximum(nrm[cand] + qn[q] - 2.0 * s, 0.0))
            s = s * b[q]
            out.append(cand[np.lexsort((cand, -s))[:R]])
        return out
    tops = lists(Qd, qn, b)
    if mut == "unmasked_lanes":
        lanes = (nq + E.TILE_Q - 1) // E.TILE_Q * E.TILE_Q
        if lanes > nq:
            ghost = lists(np.zeros((1, dim)), np.zeros(1), np.ones(1))[0]
            for q in range(nq, lanes):
                tops[q % nq] = ghost
    return tops


def first_pass_model(rows, qv, bst, metric):
    """(m, delta) f64 [n_rows]: the model score of the first pass for every row and the bound on the device's
    distance from it (module docstring)"""
    rows, qv = np.ascontiguousarray(rows, F32), np.ascontiguousarray(qv, F32)
    xb, qb = bf16_round(rows).astype(F64), bf16_round(qv).astype(F64)
    s, A = xb @ qb, np.abs(xb) @ np.abs(qb)
    n = dim_pad(rows.shape[1])
    g = n * U / (1.0 - n * U)
    ab = abs(float(bst))
    if metric == 0:
        return s * float(bst), ab * (g * A + U * (np.abs(s) + g * A))
    nrm = norms_l2r(rows).astype(F64)
    qn = float(norms_l2r(qv[None, :])[0])
    D = nrm + qn - 2.0 * s
    e1 = U * (nrm + qn)
    eD = 2 * g * A + e1 + U * (np.abs(D) + 2 * g * A + e1)
    root = np.sqrt(np.maximum(D, 0.0))
    with np.errstate(divide="ignore"):
        es = np.minimum(np.sqrt(eD), np.where(root > 0, eD / np.where(root > 0, root, 1.0), np.inf))
    return -root * float(bst), ab * (es + 2 * U * (root + es))


# ------------------------------------------------------------------ grid values (k / 16, |k| <= 8)
BOOSTS = (1.0, 2.0, -1.0, 0.5)


def _grid(rng, shape, kmax=8):
    return (rng.integers(-kmax, kmax + 1, size=shape) / 16.0).astype(F32)


def grid_store(rng, n_docs, dim, metric, p_missing=0.15, tail=False):
    """a segment's store of grid rows, out of doc order; its first and last doc have a vector.  tail: the last
    component is +-8/16 and every other one at most 7/16 in magnitude"""
    have = rng.random(n_docs) >= p_missing
    have[0] = have[-1] = True
    n_rows = int(have.sum())
    offs = np.full(n_docs, NOVEC, np.uint32)
    offs[np.nonzero(have)[0]] = rng.permutation(n_rows)
    vals = _grid(rng, (n_rows, dim), 7 if tail else 8)
    if tail:
        vals[:, -1] = rng.choice(np.array([-0.5, 0.5], F32), size=n_rows)
    return metric, offs, vals


def distinct_grid_queries(rng, nq, dim, kmax=8):
    """nq pairwise distinct grid vectors"""
    qs = np.unique(_grid(rng, (4 * nq + 8, dim), kmax), axis=0)
    assert len(qs) >= nq
    return qs[rng.permutation(len(qs))[:nq]].astype(F32)


# ------------------------------------------------------------------ a. the big world, bf16-exact
BIG_ORDERS = E.BIG_ORDERS
BIG_METRICS = (0, 1)
BIG_TOPK = (1, 32, 33, 64)                                   # cand = refine
BIG_STORE = ((65, 65), (33, 65), (64, 4000), (4000, 4000))   # (cand, refine)
BIG_L2_Q = np.array([[3, -2, 1, 5], [-5, 7, 2, -3], [3, -2, 1, 5]], F32)   # boosts 1, 2, -1
BIG_BOOST = np.array([[1.0], [2.0], [-1.0]], F32)
_cache = {}


def _two_squares(limit=4096):
    t = np.full((limit, 2), -1, np.int64)
    for c in range(64):
        for d in range(c + 1):
            if c * c + d * d < limit:
                t[c * c + d * d] = (c, d)
    return t


def four_squares(n):
    """y int [len(n), 4] with y.y = n, components below 232: two components near sqrt(n / 2) and sqrt of the rest, the
    remainder a sum of two squares from a table.  n = 4^k m (m no multiple of 16) is solved as 2^k y(m): a multiple of a high power of 4 has
    few representations of its own"""
    full = np.asarray(n, np.int64)
    n, scale = full.copy(), np.ones(len(full), np.int64)
    while np.any((n % 16 == 0) & (n > 0)):
        even = (n % 16 == 0) & (n > 0)
        n[even] //= 4
        scale[even] *= 2
    t2 = _two_squares()
    y = np.zeros((len(n), 4), np.int64)
    done = np.zeros(len(n), bool)
    a0 = np.sqrt(n / 2.0).astype(np.int64)
    for da in range(10):
        a = np.maximum(a0 - da, 0)
        r = n - a * a
        b0 = np.sqrt(r.astype(F64)).astype(np.int64)
        b0 -= (b0 * b0 > r)
        for db in range(10):
            b = np.maximum(b0 - db, 0)
            r2 = r - b * b
            hit = ~done & (r2 < len(t2))
            hit[hit] = t2[r2[hit], 0] >= 0
            y[hit] = np.stack([a[hit], b[hit], t2[r2[hit], 0], t2[r2[hit], 1]], axis=1)
            done |= hit
    y *= scale[:, None]
    assert done.all() and np.array_equal((y * y).sum(1), full) and y.max() < 232
    return y


def big_rows(order, metric):
    """the row of every flat doc of the big layout.
    cosine: m < 2^18 as three 6-bit digits (a, b, c, 0); against s (2^12, 2^6, 1, 0) a doc scores m s.
      "asc" m = flat + 1, "desc" m = total - flat, "tied" m = 32768.
    L2: BIG_L2_Q[0] + y with y.y = n (four_squares), signs of y from the bits of flat: the squared distance to
      query 0 is n.  "asc" n = total - flat (every doc is nearer than all before it), "desc" n = flat + 1, "tied" n = 9."""
    total = sum(E.BIG_DOCS)
    flat = np.arange(total, dtype=np.int64)
    m = {"asc": flat + 1, "desc": total - flat, "tied": np.full(total, 32768 if metric == 0 else 9)}[order]
    if metric == 1 and order != "tied":
        m = total + 1 - m
    if metric == 0:
        return np.stack([m >> 12, (m >> 6) & 63, m & 63, np.zeros_like(m)], axis=1).astype(F32)
    sign = 1 - 2 * ((flat[:, None] >> np.arange(4)[None, :]) & 1)
    return (BIG_L2_Q[0].astype(np.int64)[None, :] + four_squares(m) * sign).astype(F32)


def big_world(order, metric):
    """E.big_world's layout (segments, missing vectors, row order, tombstones) with bf16-exact rows"""
    key = ("big", order, metric)
    if key not in _cache:
        L = E.exact_world(E.BIG_DOCS, E.BIG_DIM, "tied", seed=4100, dels=E.BIG_DELS)
        rows = big_rows(order, metric)
        stores, base = [], 0
        for n, (_, offs, vals) in zip(L.n_docs, L.stores):
            docs = np.nonzero(offs != NOVEC)[0]
            v = np.zeros_like(vals)
            v[offs[docs]] = rows[base + docs]
            stores.append((metric, offs, v))
            base += n
        _cache[key] = E.VecWorld(E.BIG_DOCS, stores, E.BIG_DELS)
    return _cache[key]


def big_queries(metric):
    if metric == 0:
        qv = np.array([[s * 4096.0, s * 64.0, s, 0.0] for s in (1.0, 2.0, 0.5)], F32)
    else:
        qv = BIG_L2_Q.copy()
    return qv, BIG_BOOST.copy()


def big_lists(order, metric):
    """the big world's queries, boosts and every query's whole sorted list, computed once"""
    key = ("biglists", order, metric)
    if key not in _cache:
        W = big_world(order, metric)
        qv, boost = big_queries(metric)
        _cache[key] = (qv, boost, E.sorted_lists([W.stores], [0], qv, boost, W.live_masks))
    return _cache[key]


# ------------------------------------------------------------------ b. dimension steps
DIMS = (1, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 1024)
DIM_CANDS = (20, 70)
SMALL_DIM = 3      # the field ahead of the clause under test in the two-clause call: its offset is 3 floats


def dim_world(dim, metric):
    """about 300 docs: odd dims in three segments whose middle one lacks the field, even dims in two.  Grid rows and
    queries whose last component is +-8/16, the largest in magnitude; boosts 1, 2, -1, 1/2.
    -> W, qv [4, dim], boost, the stores of the 3-dimension cosine field"""
    key = ("dim", dim, metric)
    if key not in _cache:
        rng = np.random.default_rng(7000 + 2000 * metric + dim)
        n_docs = (170, 40, 90) if dim % 2 else (170, 130)
        stores = [None if len(n_docs) == 3 and s == 1 else grid_store(rng, n, dim, metric, tail=True)
                  for s, n in enumerate(n_docs)]
        W = E.VecWorld(n_docs, stores, {0: {3, 7, 100, 169}, len(n_docs) - 1: set(range(0, 90, 5))})
        qv = _grid(rng, (4, dim), 7)
        qv[:, -1] = (0.5, -0.5, 0.5, -0.5)
        if dim == 1:
            qv[:, 0] = (0.5, -0.5, 0.25, -0.25)
        boost = np.array(BOOSTS, F32)[:, None]
        small = [grid_store(rng, n, SMALL_DIM, 0, p_missing=0.3) for n in n_docs]
        _cache[key] = (W, qv, boost, small)
    return _cache[key]


# ------------------------------------------------------------------ c. query tiles
QUERY_TILE_NQS = E.QUERY_TILE_NQS
QUERY_TILE_CANDS = (8, 100)


def query_tile_world(metric):
    key = ("qtile", metric)
    if key not in _cache:
        rng = np.random.default_rng(7100 + metric)
        n_docs = (170, 130)
        W = E.VecWorld(n_docs, [grid_store(rng, n, 8, metric) for n in n_docs], {0: {4, 9, 169}, 1: {0, 64}})
        _cache[key] = W
    return _cache[key]


def query_tile_queries(nq):
    """pairwise distinct grid queries; boosts +-(q + 1) / 64: 8 significant bits, pairwise distinct.  A cosine
    score is at most 10 bits wide here, so score * boost is exact"""
    qv = distinct_grid_queries(np.random.default_rng(7200 + nq), nq, 8)
    q = np.arange(nq)
    return qv, (((q + 1) / 64.0) * np.where(q % 2, -1.0, 1.0)).astype(F32)[:, None]


# ------------------------------------------------------------------ d. doc tiles
DOC_TILE_WORLDS = E.DOC_TILE_TOTALS + ("3seg",)
DOC_TILE_CANDS = (5, 70)


def doc_tile_world(name, metric):
    key = ("dtile", name, metric)
    if key not in _cache:
        rng = np.random.default_rng(7300 + 1000 * metric + (0 if name == "3seg" else name))
        if name == "3seg":
            n_docs = E.THREE_SEGS
            stores = [grid_store(rng, 64, 8, metric, 0.1), None, grid_store(rng, 1, 8, metric, 0.0)]
            dels = {0: {3, 40}}
        else:
            n_docs = (name,)
            stores = [grid_store(rng, name, 8, metric, 0.1 if name > 1 else 0.0)]
            dels = {0: {n for n in (2, 100) if n < name}}
        _cache[key] = E.VecWorld(n_docs, stores, dels)
    return _cache[key]


def doc_tile_queries():
    qv = distinct_grid_queries(np.random.default_rng(7400), 3, 8)
    return qv, np.array([[1.0], [2.0], [-1.0]], F32)


# ------------------------------------------------------------------ e. cosine NaN -> 0
def nan_queries():
    """E.nan_world's queries as bf16 values: (1 + q / 4, 0, .., 0); E.exact_queries' 1 + q / 256 has nine bits"""
    qv = np.zeros((4, 8), F32)
    qv[:, 0] = (1.0, 1.25, 1.5, 1.75)
    return qv, np.array([[-1.0], [1.0], [-2.0], [2.0]], F32)


# ------------------------------------------------------------------ 2. general data
GENERAL_DIMS = (65, 129, 193, 257, 1024)
GENERAL_R = (20, 64, 100)
GENERAL_DOCS = (330, 270)
GENERAL_NQ = 8
GENERAL_BOOST = (1.0, 0.5, 2.0, -1.0, 1.0, 1.5, 1.0, -2.0)
# the seed of each (dim, metric): the first from 0 whose band holds at most max(2, R // 10) docs besides the R-th
# for every query and every R (test_vector_approx_edge_worlds.test_general_bands recomputes the bands)
GENERAL_SEEDS = {(d, m): 0 for d in GENERAL_DIMS for m in (0, 1)}
GENERAL_SEEDS[1024, 1] = 1


def general_band_limit(R):
    return max(2, R // 10)


def general_world(dim, metric, seed=None):
    """600 docs in two segments, a tenth without a vector, tombstones; unit vectors (cosine) or standard normal
    ones (L2); 8 queries of the same kind.  -> W, qv, boost"""
    seed = GENERAL_SEEDS[dim, metric] if seed is None else seed
    key = ("general", dim, metric, seed)
    if key not in _cache:
        rng = np.random.default_rng(7500 + 100_000 * seed + 10 * dim + metric)
        stores = [V._store(rng, n, dim, metric, p_missing=0.1) for n in GENERAL_DOCS]
        W = E.VecWorld(GENERAL_DOCS, stores, {0: {1, 5, 17, 329}, 1: {0, 200}})
        qv = V._unit(rng, GENERAL_NQ, dim) if metric == 0 else rng.standard_normal((GENERAL_NQ, dim)).astype(F32)
        _cache[key] = (W, qv, np.array(GENERAL_BOOST, F32)[:, None])
    return _cache[key]


def general_model(W, qv, boost, metric):
    """per query (keys [(segment, doc)], m, delta) over the live docs with a vector, in flat order"""
    rows, ok = flat_view(W)
    flats = np.nonzero(ok)[0]
    keys = flat_keys(W, flats)
    return [(keys,) + first_pass_model(rows[flats], qv[q], boost[q, 0], metric) for q in range(len(qv))]


def general_band(m, delta, R):
    """(t, must [n] bool: has to be returned, never [n] bool: must not be, band [n] bool: free) of one query"""
    t = np.sort(m)[::-1][R - 1]
    w = delta + delta.max()
    return t, m - t > w, t - m > w, np.abs(m - t) <= w
