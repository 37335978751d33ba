"""slg_index_train_vector_field on the device against the parent's own assignment combined with the numpy update.

The yardstick of every step: a second GpuIndex over the same store is clustered with cluster_vector_field(C_{t-1})
(code that predates the training call), its lists are fetched, and C_t = tests/ivf_train_ref.update(...) in numpy,
operation by operation as the header states it.  After T steps the device call's centroids must equal the
reference's bit for bit, the lists must be equal and the stats must equal the reference's counts.  No tolerance
appears anywhere in this file."""
import numpy as np
import pytest

from tests import ivf_train_ref as R
from tests.test_gpu_vector_ivf import same, seg_of
from tests.test_gpu_vector_search import NOVEC, _seg, _store, _unit

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def dense_store(rng, vals, metric, n_missing=0):
    """(metric, offsets, values): every row referred to by one doc, rows out of doc order, n_missing docs without"""
    n_rows = len(vals)
    n_docs = n_rows + n_missing
    have = np.ones(n_docs, bool)
    have[rng.choice(n_docs, n_missing, replace=False)] = False
    offs = np.full(n_docs, NOVEC, np.uint32)
    offs[np.nonzero(have)[0]] = rng.permutation(n_rows)
    return metric, offs, np.ascontiguousarray(vals, F32)


def wide(rng, shape, big_exp=0):
    """f32 columns whose f64 sum depends on the order of the additions by far more than an f32 ulp of the result:
    half of a column's values are +-2^big_exp in equal numbers (they cancel exactly, and while they have not, the
    running sum drops the low bits of what is added), the others are normal values 2^40 times smaller"""
    shape = (shape, 1) if isinstance(shape, int) else shape
    n, cols = shape
    out = (rng.standard_normal(shape) * 2.0 ** (big_exp - 40)).astype(F32)
    for c in range(cols):
        idx = rng.permutation(n)[: 2 * (n // 4)]
        out[idx[: len(idx) // 2], c] = 2.0 ** big_exp
        out[idx[len(idx) // 2:], c] = -(2.0 ** big_exp)
    return out


class Ref:
    """the reference loop over a second index of the same store"""

    def __init__(self, store, deleted=None):
        import searchlite_amd as sa
        self.metric, self.offs, self.vals = store
        seg = seg_of(len(self.offs), store)
        if deleted is not None:
            seg.set_deleted([int(d) for d in deleted])
        self.ix = sa.GpuIndex([seg])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ix.close()

    def assign(self, cents):
        self.ix.cluster_vector_field(0, [np.ascontiguousarray(cents, F32)])
        begin, docs, _ = self.ix.fetch_vector_lists(0, 0, self.vals.shape[1])
        return begin, docs, R.row_lists(begin, docs, self.offs, len(self.vals))

    def train(self, init, iters, stop=True):
        return R.train(self.assign, self.vals, self.offs, init, self.metric, iters, stop)


def start_rows(vals, n_lists):
    return np.ascontiguousarray(vals[[(i * len(vals)) // n_lists for i in range(n_lists)]], F32)


def device_train(store, n_lists, iters, init, deleted=None):
    import searchlite_amd as sa
    seg = seg_of(len(store[1]), store)
    if deleted is not None:
        seg.set_deleted([int(d) for d in deleted])
    with sa.GpuIndex([seg]) as ix:
        stats = ix.train_vector_field(0, [(n_lists, iters, init)])
        assert len(stats) == 1
        begin, docs, cents = ix.fetch_vector_lists(0, 0, store[2].shape[1])
    return cents, begin, docs, stats[0]


def agree(got, want, what):
    """centroids bit for bit, equal lists and, where both sides carry them, equal stats"""
    if len(got) > 3 and len(want) > 3:
        assert got[3] == want[3], f"{what}: stats {got[3]} != {want[3]}"
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), f"{what}: the lists differ"
    assert got[0].shape == want[0].shape
    bad = np.nonzero(bits(got[0]) != bits(want[0]))
    assert len(bad[0]) == 0, f"{what}: {len(bad[0])} centroid words differ, first at list {bad[0][0]} dim {bad[1][0]}"


def check(store, n_lists, iters, init, what, deleted=None):
    """init None: the device starts from rows of the store, the reference from the same rows passed explicitly"""
    got = device_train(store, n_lists, iters, init, deleted)
    with Ref(store, deleted) as ref:
        want = ref.train(start_rows(store[2], n_lists) if init is None else init, iters)
    agree(got, want, what)
    return got, want


# ---- 1. the dims at which the kernels take another path, both metrics ----
# vs_ivf_sum_kernel: dim d belongs to thread d mod 256, a thread carries 1 .. 4 dims of a group of 1024 side by side
# (255 / 256 / 257: one or two; 513 and 768: three; 1024: four; 1025: a second group); vs_ivf_centroid_kernel: tiles of
# 2048 dims with s carried from tile to tile (2048 / 2049).
DIM_EDGES = (255, 256, 511, 512, 767, 768, 1023, 1024, 2047, 2048)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("dim", [1, 7, 33, 100, 255, 256, 257, 513, 768, 1024, 1025, 2048, 2049])
def test_dims_bit_for_bit(dim, metric):
    rng = np.random.default_rng(10 * dim + metric)
    n = 300
    vals = _unit(rng, n, dim) if metric == 0 else rng.standard_normal((n, dim)).astype(F32)
    # order-dependent sums in the last dim and on both sides of every pass, group and tile boundary below it
    cols = sorted({dim - 1} | {d for d in DIM_EDGES if d < dim})
    vals[:, cols] = wide(rng, (n, len(cols)), -6)
    store = dense_store(rng, vals, metric, n_missing=20)
    got, want = check(store, 5, 3, None, f"dim {dim} metric {metric}")
    assert got[3]["iters_run"] >= 1 and not np.array_equal(bits(got[0]), bits(start_rows(vals, 5)))
    moved = (bits(got[0]) != bits(start_rows(vals, 5))).any(axis=0)
    assert moved[cols].all(), "an order-dependent column was left as it started in every list"


# ---- 2. n_lists 1, 2 and one past the scan's 128-doc tile of centroids; one list sums 600 rows in three chunks ----
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("n_lists", [1, 2, 129])
def test_n_lists_bit_for_bit(n_lists, metric):
    rng = np.random.default_rng(7 * n_lists + metric)
    n, dim = 600, 6
    vals = wide(rng, (n, dim))
    store = dense_store(rng, vals, metric, n_missing=5)
    got, want = check(store, n_lists, 2, None, f"n_lists {n_lists} metric {metric}")
    if n_lists == 1:
        # the chunked order is not the straight one: a sum over the 600 rows in doc order gives other bytes
        order = store[1][store[1] != NOVEC]
        straight = np.zeros(dim)
        for r in order:
            straight += vals[r].astype(np.float64)
        assert got[3] == dict(iters_run=1, moved=0, empty_lists=0, max_len=600)
        if metric == 1:
            assert not np.array_equal(bits((straight / 600).astype(F32)), bits(got[0][0]))


# ---- 3. list lengths at the chunk boundaries, in one store ----
LENGTHS = [257, 0, 1, 513, 255, 256]


def _chunk_world(rng, metric):
    dim = 9
    scale = F32(1.0) if metric == 0 else F32(10.0)
    cents = np.eye(dim, dtype=F32)[:6] * scale
    cents[1] = -np.ones(dim, F32) * scale          # far from every row: its list stays empty
    rows = []
    for l, n in enumerate(LENGTHS):
        v = np.tile(cents[l], (n, 1))
        v[:, :6] += (rng.standard_normal((n, 6)) * 0.01).astype(F32)
        v[:, 6:] = wide(rng, (n, 3), -6)                 # small next to the rest, summed in an order-dependent way
        rows.append(v)
    return dense_store(rng, np.concatenate(rows), metric, n_missing=9), cents


@pytest.mark.parametrize("metric", [0, 1])
def test_list_lengths_at_the_chunk_boundaries(metric):
    rng = np.random.default_rng(40 + metric)
    store, cents = _chunk_world(rng, metric)
    # on the host alone: every row is far nearer its own centroid than any other, in f64
    v, c = store[2].astype(np.float64), cents.astype(np.float64)
    score = v @ c.T if metric == 0 else -np.linalg.norm(v[:, None, :] - c[None], axis=2)
    best = np.sort(score, axis=1)
    assert ((best[:, -1] - best[:, -2]) > 0.5).all()
    assert np.bincount(np.argmax(score, axis=1), minlength=6).tolist() == LENGTHS
    got, want = check(store, 6, 2, cents, f"chunk boundaries, metric {metric}")
    assert np.diff(want[1].astype(np.int64)).tolist() == LENGTHS
    assert got[3] == dict(iters_run=1, moved=0, empty_lists=1, max_len=513)
    assert np.array_equal(bits(got[0][1]), bits(cents[1]))   # the empty list kept its centroid
    assert (bits(got[0][[0, 2, 3, 4, 5]]) != bits(cents[[0, 2, 3, 4, 5]])).any(axis=1).all()
    # all steps of an unstopped run too: lengths stay, the centroids are those of step 1
    with Ref(store) as ref:
        agree(got, ref.train(cents, 2, stop=False)[:3] + (got[3],), "without the stop rule")


# ---- 4. past one 65 536-row launch of the assignment and of the moved counter ----
def test_a_store_of_65537_rows():
    rng = np.random.default_rng(4)
    n = 65537
    vals = (rng.standard_normal((n, 2)) + np.array([[3.0, 0.0]]) * rng.integers(0, 3, (n, 1))).astype(F32)
    store = dense_store(rng, vals, 1)
    init = np.array([[0.5, 0.0], [2.0, 0.5], [7.0, -1.0]], F32)
    got, want = check(store, 3, 2, init, "65537 rows")
    assert got[3]["iters_run"] == 2 and 0 < got[3]["moved"] < n
    # the last row, alone in its launch of the assignment, is the only row that moves in step 2: with the centroids
    # (-1, 0) and (10, 0) it is nearer the second (5.3 < 5.7), with the means (0, 0) and ~(10, 0) nearer the first
    far = np.zeros((n, 2), F32)
    far[: n // 2] = [10.0, 0.0]
    far[-1] = [4.7, 0.0]
    init2 = np.array([[-1.0, 0.0], [10.0, 0.0]], F32)
    got2, want2 = check((1, np.arange(n, dtype=np.uint32), far), 2, 2, init2, "65537 rows, the last one moves")
    assert got2[3]["iters_run"] == 2 and got2[3]["moved"] == 1


# ---- 5. docs without a vector, a shared row, tombstones, duplicates of a centroid, equal scores ----
@pytest.mark.parametrize("metric", [0, 1])
def test_store_with_every_irregularity(metric):
    rng = np.random.default_rng(50 + metric)
    dim, n = 12, 400
    vals = np.abs(_unit(rng, n, dim)) if metric == 0 else rng.standard_normal((n, dim)).astype(F32)
    vals[10] = vals[3]                      # rows that are exact duplicates of centroid 0 (= row 3)
    vals[11] = vals[3]
    _, offs, vals = dense_store(rng, vals, metric, n_missing=40)
    free = np.nonzero(offs == NOVEC)[0]
    offs[free[0]] = offs[np.nonzero(offs != NOVEC)[0][5]]   # two docs share one row
    assert (offs == NOVEC).sum() == 39
    deleted = np.nonzero(offs != NOVEC)[0][::7]             # tombstoned docs: assigned and summed all the same
    init = np.ascontiguousarray(np.stack([vals[3], vals[3], vals[50], vals[90], vals[91]]))  # lists 0, 1 tie: -> 0
    store = (metric, offs, vals)
    got, want = check(store, 5, 3, init, f"irregular store, metric {metric}", deleted=deleted)
    undeleted = device_train(store, 5, 3, init)
    agree(got, undeleted, "tombstones change nothing")
    assert int(got[1][-1]) == int((offs != NOVEC).sum()) == n + 1
    # after step 1 the tie is over, but list 1 was empty then and kept its centroid: check step 1 alone
    one = device_train(store, 5, 1, init)
    with Ref(store) as ref:
        b1, d1, _ = ref.assign(init)
    assert b1[1] == b1[2] and b1[1] - b1[0] >= 3            # list 1 empty, list 0 holds the duplicates
    assert np.array_equal(bits(one[0][1]), bits(init[1])) and not np.array_equal(bits(one[0][0]), bits(init[0]))


# ---- 6. the lists that keep their previous centroid ----
def test_a_list_that_empties_after_step_1_keeps_its_centroid():
    x = [0.0, 0.0, 0.0, 0.875, 3.125, 4.0, 4.0, 4.0]
    vals = np.array([[v, 0.0] for v in x], F32)
    vals[:, 1] = [0.01, -0.01, 0.02, 0.0, 0.0, 0.03, -0.02, 0.01]
    store = (1, np.arange(len(x), dtype=np.uint32), vals)
    init = np.array([[-1.5, 0.0], [2.0, 0.0], [5.5, 0.0]], F32)
    one = device_train(store, 3, 1, init)
    assert np.diff(one[1].astype(np.int64)).tolist() == [4, 0, 4]   # after step 1 list 1's two rows have left it
    got, want = check(store, 3, 3, init, "a list empties")
    assert np.array_equal(bits(got[0][1]), bits(one[0][1])) and got[3]["empty_lists"] == 1
    assert float(one[0][1][0]) == 2.0
    assert not np.array_equal(bits(got[0][0]), bits(one[0][0])) and not np.array_equal(bits(got[0][2]), bits(one[0][2]))


def test_a_cosine_list_of_two_opposite_rows_keeps_its_centroid():
    """Two opposite rows share a list only where every centroid ties for each of them: (1, 0, 0) scores 0.5 against
    both centroids and (-1, 0, 0) scores -0.5 (sums without a signed zero), so both go to list 0, whose mean is 0."""
    rng = np.random.default_rng(61)
    h = F32(np.sqrt(0.75))
    init = np.array([[0.5, h, 0.0], [0.5, 0.0, h]], F32)
    near = init[1][None, :] + _unit(rng, 30, 3) * F32(0.05)
    near[:, 1] = -np.abs(near[:, 1]) - F32(0.05)                # (below list 1's score against list 0)
    near = (near / np.linalg.norm(near, axis=1, keepdims=True)).astype(F32)
    vals = np.concatenate([np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], F32), near])
    store = (0, np.arange(len(vals), dtype=np.uint32), vals)
    with Ref(store) as ref:
        b0, d0, _ = ref.assign(init)
    assert np.diff(b0.astype(np.int64)).tolist() == [2, 30] and d0[:2].tolist() == [0, 1], (b0, d0[:4])
    got, want = check(store, 2, 1, init, "s == 0")              # the update of that assignment
    assert got[3]["iters_run"] == 1
    assert np.array_equal(bits(got[0][0]), bits(init[0])) and not np.array_equal(bits(got[0][1]), bits(init[1]))
    check(store, 2, 3, init, "s == 0, further steps")            # (list 1's new centroid then breaks the tie)


@pytest.mark.parametrize("metric", [0, 1])
def test_a_list_holding_a_nan_row_keeps_its_centroid(metric):
    rng = np.random.default_rng(62 + metric)
    dim = 5
    vals = np.abs(_unit(rng, 80, dim)) if metric == 0 else rng.standard_normal((80, dim)).astype(F32)
    vals[17, 2] = np.nan
    store = (metric, np.arange(80, dtype=np.uint32), vals)
    init = np.ascontiguousarray(vals[[1, 30, 60]])
    got, want = check(store, 3, 2, init, f"NaN row, metric {metric}")
    holder = [l for l in range(3) if 17 in got[2][got[1][l]:got[1][l + 1]].tolist()]
    one = device_train(store, 3, 1, init)
    holder1 = [l for l in range(3) if 17 in one[2][one[1][l]:one[1][l + 1]].tolist()]
    with Ref(store) as ref:
        b0, d0, _ = ref.assign(init)
    holder0 = [l for l in range(3) if 17 in d0[b0[l]:b0[l + 1]].tolist()]
    assert len(holder0) == 1, "the NaN row is in no list: the case checks nothing"
    h = holder0[0]
    assert np.array_equal(bits(one[0][h]), bits(init[h]))       # its list kept C_0 in step 1
    others = [l for l in range(3) if l != h]
    assert all(not np.array_equal(bits(one[0][l]), bits(init[l])) for l in others)
    assert not np.isnan(got[0]).any() and holder == holder1 == holder0


# ---- 7. the start from rows of the store ----
@pytest.mark.parametrize("metric", [0, 1])
def test_start_from_store_rows(metric):
    import searchlite_amd as sa
    from searchlite_amd import _native as N
    rng = np.random.default_rng(70 + metric)
    dim = 10
    store = _store(rng, 50, dim, metric)
    rows = len(store[2])
    for n_lists in (1, 4, rows - 1, rows):
        a = device_train(store, n_lists, 2, None)
        b = device_train(store, n_lists, 2, start_rows(store[2], n_lists))
        agree(a, b, f"init None, n_lists {n_lists}")
        zero = device_train(store, n_lists, 0, None)
        assert np.array_equal(bits(zero[0]), bits(start_rows(store[2], n_lists)))
    with sa.GpuIndex([seg_of(50, store)]) as ix:
        with pytest.raises(N.SlgError) as e:
            ix.train_vector_field(0, [(rows + 1, 2)])
        assert e.value.code == N.ERR_INVALID and "rows" in str(e.value)
        assert ix.fetch_vector_lists(0, 0, dim) is None
        init = rng.standard_normal((rows + 1, dim)).astype(F32)
        st = ix.train_vector_field(0, [(rows + 1, 2, init)])[0]
        assert st["empty_lists"] >= 1 and len(ix.fetch_vector_lists(0, 0, dim)[2]) == rows + 1
    with Ref(store) as ref:
        agree(device_train(store, rows + 1, 2, init), ref.train(init, 2), "more lists than rows, with init")


# ---- 8. iters 0; 9. the guarantee ----
def _state(ix, dim, segs=(0,)):
    out = []
    for s in segs:
        got = ix.fetch_vector_lists(0, s, dim)
        out.append(None if got is None else tuple(a.tobytes() for a in got))
    return out


@pytest.mark.parametrize("metric", [0, 1])
def test_iters_0_is_cluster_vector_field_and_the_guarantee(metric):
    import searchlite_amd as sa
    rng = np.random.default_rng(80 + metric)
    dim = 33
    store = _store(rng, 500, dim, metric)
    init = np.ascontiguousarray(store[2][rng.choice(len(store[2]), 7, replace=False)])
    with sa.GpuIndex([seg_of(500, store)]) as ix, sa.GpuIndex([seg_of(500, store)]) as fresh:
        st = ix.train_vector_field(0, [(7, 0, init)])[0]
        fresh.cluster_vector_field(0, [init])
        assert _state(ix, dim) == _state(fresh, dim)
        lens = np.diff(ix.fetch_vector_lists(0, 0, dim)[0].astype(np.int64))
        assert st == dict(iters_run=0, moved=0, empty_lists=int((lens == 0).sum()), max_len=int(lens.max()))
        for iters in (1, 4):
            st = ix.train_vector_field(0, [(7, iters, init)])[0]
            begin, docs, cents = ix.fetch_vector_lists(0, 0, dim)
            assert st["iters_run"] >= 1 and not np.array_equal(bits(cents), bits(init))
            fresh.cluster_vector_field(0, [cents])
            assert _state(ix, dim) == _state(fresh, dim), f"iters {iters}"


# ---- 10. the early stop ----
def _blobs(rng, metric, n_blobs=6, per=60, dim=8):
    centres = np.eye(dim, dtype=F32)[:n_blobs] * F32(1.0 if metric == 0 else 20.0)
    v = np.repeat(centres, per, axis=0) + (rng.standard_normal((n_blobs * per, dim)) * 0.05).astype(F32)
    if metric == 0:
        v = v / np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(F32), centres


@pytest.mark.parametrize("metric", [0, 1])
def test_early_stop(metric):
    rng = np.random.default_rng(90 + metric)
    vals, centres = _blobs(rng, metric)
    store = dense_store(rng, vals, metric, n_missing=11)
    init = np.ascontiguousarray(vals[::60] * F32(0.9) + vals[30::60][::-1] * F32(0.1))
    got = device_train(store, 6, 50, init)
    assert 1 <= got[3]["iters_run"] < 50 and got[3]["moved"] == 0
    with Ref(store) as ref:
        agree(got, ref.train(init, 50), "with the stop rule")
        T = got[3]["iters_run"]
        more = ref.train(init, T + 6, stop=False)
        agree(got[:3], more[:3], "six further steps without the stop rule")
    assert np.diff(got[1].astype(np.int64)).tolist() == [60] * 6


# ---- 11. searching a trained field ----
@pytest.mark.parametrize("metric", [0, 1])
def test_search_over_a_trained_field(metric):
    import searchlite_amd as sa
    rng = np.random.default_rng(110 + metric)
    vals, centres = _blobs(rng, metric)
    store = dense_store(rng, vals, metric, n_missing=20)
    qv = np.ascontiguousarray(vals[rng.choice(len(vals), 40, replace=False)] + F32(0.001))
    seg = seg_of(len(store[1]), store)
    seg.set_deleted([1, 2, 3])
    with sa.GpuIndex([seg]) as ix:
        st = ix.train_vector_field(0, [(6, 10)])[0]
        assert st["empty_lists"] == 0
        for cand, k_out in ((10, 10), (64, 30)):
            exact = ix.vector_search([0], qv, 0.0, cand, k_out)
            for nprobe in (6, 7, 256):
                same(ix.vector_search_ivf([0], qv, 0.0, cand, nprobe, k_out), exact, f"nprobe {nprobe}")
        exact = ix.vector_search([0], qv, 0.0, 5, 5)
        one = ix.vector_search_ivf([0], qv, 0.0, 5, 1, 5)
        assert (one[4] >= 1).all()
        assert np.array_equal(one[0][:, 0], exact[0][:, 0]) and np.array_equal(bits(one[2][:, 0]), bits(exact[2][:, 0]))


# ---- 12. lifecycle ----
def test_lifecycle():
    import searchlite_amd as sa
    from searchlite_amd import _native as N
    rng = np.random.default_rng(120)
    dim, metric = 16, 0
    n_docs = [300, 200, 150, 120]
    stores = [_store(rng, n, dim, metric) for n in n_docs[:3]] + [None]
    qv = _unit(rng, 9, dim)
    c1 = np.ascontiguousarray(stores[1][2][:3])

    def trained_alone(s, n_lists, iters):
        return tuple(a.tobytes() for a in (lambda t: (t[1], t[2], t[0]))(device_train(stores[s], n_lists, iters, None)))

    with sa.GpuIndex([seg_of(n, st) for n, st in zip(n_docs, stores)]) as ix:
        ix.cluster_vector_field(0, [None, c1, None, None])
        kept = _state(ix, dim, range(4))
        stats = ix.train_vector_field(0, [(5, 3), N.KEEP_VECTOR_LISTS, None, None])
        assert stats[1] == stats[2] == stats[3] == dict(iters_run=0, moved=0, empty_lists=0, max_len=0)
        assert stats[0]["iters_run"] >= 1
        now = _state(ix, dim, range(4))
        assert now[1] == kept[1] and now[2] is None and now[3] is None
        assert now[0] == trained_alone(0, 5, 3)                 # a segment trains on its own store alone
        # different n_lists per segment in one call; a segment without vectors cannot be trained
        with pytest.raises(N.SlgError) as e:
            ix.train_vector_field(0, [N.KEEP_VECTOR_LISTS, N.KEEP_VECTOR_LISTS, None, (2, 1)])
        assert e.value.code == N.ERR_INVALID and _state(ix, dim, range(4)) == now
        for bad in ([(5, 3)], [(5, 3)] * 5):
            with pytest.raises(N.SlgError) as e:
                ix.train_vector_field(0, bad)
            assert e.value.code == N.ERR_INVALID
        with pytest.raises(N.SlgError) as e:
            ix.train_vector_field(1, [(5, 3), None, None, None])    # no such field
        assert e.value.code == N.ERR_INVALID
        with pytest.raises(N.SlgError) as e:
            ix.train_vector_field(0, [(65537, 3), None, None, None])
        assert e.value.code == N.ERR_UNSUPPORTED and _state(ix, dim, range(4)) == now
        q1 = np.ascontiguousarray(qv[:1])
        with ix.prepare(np.array([0, 1], np.uint32), np.zeros((1, 4), np.uint32), np.ones(1, F32), 5,
                        hybrid=True) as b:  # (term 0 of each of the four segments)
            hy_before = b.hybrid([0], q1, 0.5, 5, 5)
            stats = ix.train_vector_field(0, [N.KEEP_VECTOR_LISTS, (4, 2), (7, 2), None])
            same(b.hybrid([0], q1, 0.5, 5, 5), hy_before, "a hybrid batch prepared before the training call")
        now = _state(ix, dim, range(4))
        assert now[0] == trained_alone(0, 5, 3) and now[1] == trained_alone(1, 4, 2) and now[2] == trained_alone(2, 7, 2)
        exact = ix.vector_search([0], qv, 0.2, 15, 16)
        same(ix.vector_search_ivf([0], qv, 0.2, 15, 16, 16), exact, "all lists probed")
        # tombstones after training: the lists stay, the results follow
        dbits = np.zeros(300, bool)
        dbits[[int(d) for q in range(9) for d, s in zip(exact[0][q, :2], exact[1][q, :2]) if s == 0] + [1]] = True
        ix.update_deleted(0, np.packbits(dbits, bitorder="little"), float(300 - dbits.sum()))
        assert _state(ix, dim, range(4)) == now
        after = ix.vector_search([0], qv, 0.2, 15, 16)
        same(ix.vector_search_ivf([0], qv, 0.2, 15, 16, 16), after, "update_deleted")
        assert not np.array_equal(after[0], exact[0])
        # a new segment is unclustered, scanned whole, and can be trained alone without its vectors on the host
        st4 = _store(rng, 90, dim, metric)
        assert ix.add_segment(seg_of(90, st4)) == 4
        assert _state(ix, dim, range(5)) == now + [None]
        same(ix.vector_search_ivf([0], qv, 0.2, 15, 1, 16),
             ix.vector_search_ivf([0], qv, 0.2, 15, 1, 16), "deterministic")
        got = ix.vector_search_ivf([0], qv, 0.2, 15, 1, 16)
        assert (got[1] == 4).any()
        K = N.KEEP_VECTOR_LISTS
        stats = ix.train_vector_field(0, [K, K, K, K, (3, 2)])
        stores.append(st4)
        assert _state(ix, dim, range(5)) == now + [trained_alone(4, 3, 2)]
        same(ix.vector_search_ivf([0], qv, 0.2, 15, 19, 16), ix.vector_search([0], qv, 0.2, 15, 16), "five segments")
        # remove_segment drops that segment's lists, the others keep theirs
        full = _state(ix, dim, range(5))
        ix.remove_segment(1)
        assert _state(ix, dim, range(4)) == [full[0], full[2], full[3], full[4]]
        same(ix.vector_search_ivf([0], qv, 0.2, 15, 15, 16), ix.vector_search([0], qv, 0.2, 15, 16), "after remove")
        # n_lists 0 unclusters
        ix.train_vector_field(0, [None, K, K, K])
        assert _state(ix, dim, range(4)) == [None, full[2], full[3], full[4]]


# ---- 13. the scratch of the loop is gone when the call returns ----
def test_nothing_of_the_training_scratch_is_left_in_the_pool():
    """The loop's work areas are not pooled blocks: they are freed when the call returns, so draining the pool right
    after the call frees exactly what draining it before the call left behind: nothing."""
    import searchlite_amd as sa
    rng = np.random.default_rng(130)
    dim = 40
    store = _store(rng, 3000, dim, 0)
    qv = _unit(rng, 5, dim)
    with sa.GpuIndex([seg_of(3000, store)]) as ix:
        ix.vector_search([0], qv, 0.0, 5, 5)
        ix.trim_pool()
        assert ix.trim_pool() == 0
        st = ix.train_vector_field(0, [(20, 4)])[0]
        assert st["iters_run"] >= 1
        assert ix.trim_pool() == 0, "the training call left blocks in the pool"
        first = _state(ix, dim)
        ix.train_vector_field(0, [(20, 4)])
        assert ix.trim_pool() == 0 and _state(ix, dim) == first
        same(ix.vector_search_ivf([0], qv, 0.0, 5, 20, 5), ix.vector_search([0], qv, 0.0, 5, 5), "after training")


# ---- 14. the Python wrapper's own checks ----
def test_wrapper_takes_numpy_integers_and_checks_the_width_of_init():
    import searchlite_amd as sa
    from searchlite_amd import _native as N
    rng = np.random.default_rng(140)
    dim = 6
    stores = [_store(rng, 80, dim, 0), _store(rng, 60, dim, 0)]
    with sa.GpuIndex([seg_of(80, stores[0]), seg_of(60, stores[1])]) as ix:
        first = ix.train_vector_field(0, [(np.uint32(3), np.int64(2)), None])
        assert first[0]["iters_run"] >= 1
        kept = _state(ix, dim, range(2))
        ix.train_vector_field(0, [np.uint32(N.KEEP_VECTOR_LISTS), (2, 1)])      # a numpy scalar for KEEP
        assert _state(ix, dim, range(1)) == kept[:1] and _state(ix, dim, (1,)) != [None]
        now = _state(ix, dim, range(2))
        for bad in (np.zeros((3, dim + 1), F32), np.zeros((3, dim - 1), F32)):
            with pytest.raises(ValueError):
                ix.train_vector_field(0, [(3, 1, bad), N.KEEP_VECTOR_LISTS])
        with pytest.raises(ValueError):
            ix.train_vector_field(0, [(3, 1, np.zeros((3, dim), F32)), N.KEEP_VECTOR_LISTS], dim=dim + 2)
        with pytest.raises(ValueError):
            ix.train_vector_field(0, [(3, 1, np.zeros((4, dim), F32)), N.KEEP_VECTOR_LISTS])
        assert _state(ix, dim, range(2)) == now
        ix.train_vector_field(0, [(3, 1, np.ascontiguousarray(stores[0][2][:3])), N.KEEP_VECTOR_LISTS], dim=dim)
