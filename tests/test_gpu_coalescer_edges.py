"""The request coalescer (searchlite_amd/csrc/slg_coalesce.hip) at its edges: rows with score plans and doc
filters, alone and mixed into shared batches; a bad row that must fail its own caller and nobody else; more
(k, strategy, segment count) combinations over a coalescer's life than collect at once; index updates under a
live coalescer; per-request stats and recycled batch objects; ticket misuse.

Reference, tolerance 0: a coalescer row equals the row of the same query in ONE slg_batch_prepare_plan batch over
the whole row set (same per-row plans and filters), and that batch equals the oracle (asserted once per row set
and k, so that a mismatch of a coalescer row points at the coalescer).  Equal means doc, segment, score bits and
count, and zeros past the count.

No test here may hang the suite: every call that can block in the coalescer runs on a daemon thread that is
joined with a bound of BOUND seconds (a guard, not a performance bar: the work is milliseconds).  A thread still
alive after it fails the test, and the index and its coalescers are then abandoned, not destroyed, so that
nothing more is started on the device.
"""
import ctypes as C
import math
import threading

import numpy as np
import pytest

from tests.util import assert_same_hits, random_segment

pytestmark = pytest.mark.gpu

BOUND = 60.0
SUM, DISMAX = 0, 1
PATTERN = 0xA5


@pytest.fixture(scope="module")
def sa():
    import searchlite_amd as s
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return s


def native():
    from searchlite_amd import _native as N
    return N


class Row:
    """One request: what slg_coalescer_search_plan / _submit is called with."""

    def __init__(self, tids, w, leaf=None, plan=SUM, tie=0.0, n_leaves=0, filter_id=-1):
        self.tids = np.ascontiguousarray(tids, np.uint32)  # [n_terms, n_segs]
        self.w = np.ascontiguousarray(w, np.float32)
        self.leaf = None if leaf is None else np.ascontiguousarray(leaf, np.uint32)
        self.plan, self.tie, self.n_leaves, self.filter_id = plan, tie, n_leaves, filter_id
        self.query = native().Query(len(self.w), self.tids.ctypes.data if len(self.w) else None,
                                    self.w.ctypes.data if len(self.w) else None)

    @property
    def nt(self):
        return len(self.w)

    def variant(self, **kw):
        """The same request with some arguments replaced."""
        args = dict(tids=self.tids.copy(), w=self.w.copy(), leaf=None if self.leaf is None else self.leaf.copy(),
                    plan=self.plan, tie=self.tie, n_leaves=self.n_leaves, filter_id=self.filter_id)
        args.update(kw)
        return Row(**args)

    def leaves_explicit(self):
        """(leaf per term, number of leaves) as the header defines the defaults: leaf NULL = term i is leaf i;
        n_leaves 0 = 1 + the largest leaf named."""
        leaf = np.arange(self.nt, dtype=np.uint32) if self.leaf is None else self.leaf
        derived = int(leaf.max()) + 1 if self.nt else 0
        return leaf, (self.n_leaves if self.n_leaves else derived)


class RowSet:
    """Rows and their reference: the batch API over all of them, held against the oracle once per k."""

    def __init__(self, rows):
        self.rows = list(rows)
        self._ref = {}

    def arrays(self, n_segs):
        offs = np.zeros(len(self.rows) + 1, np.uint32)
        for i, r in enumerate(self.rows):
            offs[i + 1] = offs[i] + r.nt
        terms = np.concatenate([r.tids.reshape(-1, n_segs) for r in self.rows] + [np.zeros((0, n_segs), np.uint32)])
        w = np.concatenate([r.w for r in self.rows] + [np.zeros(0, np.float32)])
        ex = [r.leaves_explicit() for r in self.rows]
        kw = dict(q_leaf=np.concatenate([e[0] for e in ex] + [np.zeros(0, np.uint32)]).astype(np.uint32),
                  q_plan=np.array([r.plan for r in self.rows], np.int32),
                  q_tie=np.array([r.tie for r in self.rows], np.float32),
                  q_nleaves=np.array([e[1] for e in ex], np.uint32))
        q_filter = np.array([r.filter_id for r in self.rows], np.int32)
        return offs, terms, w, kw, q_filter

    def batch(self, world, k, strategy=None, want_stats=False):
        sa = world.sa
        offs, terms, w, kw, qf = self.arrays(world.ix.n_segs)
        b = world.ix.prepare(offs, terms, w, k, sa.Wand if strategy is None else strategy, q_filter=qf, **kw)
        try:
            b.run()
            return b.fetch(want_stats=want_stats)
        finally:
            b.close()

    def reference(self, world, k, oracle=None):
        """(doc, seg, score, count) of the batch API; with `oracle`, asserted equal to it (k > 0)."""
        if k not in self._ref:
            got = self.batch(world, k)
            if oracle is not None and k > 0:
                offs, terms, w, kw, qf = self.arrays(world.ix.n_segs)
                ids = sorted(world.masks)
                q_filter = np.array([ids.index(f) if f >= 0 else -1 for f in qf], np.int32)
                want = oracle.search_batch_filtered(world.ix.segments, offs, terms, w, k, q_filter,
                                                    [world.masks[f] for f in ids], strategy=oracle.BM25, **kw)
                assert_same_hits(got, want, 0.0, f"batch API against the oracle, k={k}")
            self._ref[k] = got
        return self._ref[k]


class Hung(Exception):
    pass


class World:
    """Two segments (the second with tombstones) over one vocabulary, a filter that passes about half the docs
    and one that passes none, and the coalescers made on the index."""

    def __init__(self, sa, seed, updatable=False):
        self.sa, self.N, self.lib = sa, native(), native().load()
        rng = np.random.default_rng(seed)
        self.rng = rng
        self.vocab = 80
        segs = [random_segment(rng, 4000, self.vocab, 25, k1=0.9, b=0.4),
                random_segment(rng, 2500, self.vocab, 25, k1=0.9, b=0.4)]
        segs[1].set_deleted(list(range(5, segs[1].n_docs, 11)))
        self.ix = sa.GpuIndex(segs, tuning={"updatable": 1} if updatable else None)
        half = [rng.random(s.n_docs) < 0.5 for s in segs]
        none = [np.zeros(s.n_docs, bool) for s in segs]
        self.f_half, self.f_none = self.ix.add_filter(half), self.ix.add_filter(none)
        self.masks = {self.f_half: half, self.f_none: none}
        self.cos = []

    def coalescer(self, max_batch, max_wait_us=50):
        co = self.lib.slg_coalescer_create(self.ix._h, max_batch, max_wait_us)
        assert co
        self.cos.append(co)
        return co

    def destroy(self, co):
        self.cos.remove(co)
        self.lib.slg_coalescer_destroy(co)

    def abandon(self):
        """After a hang: nothing of this world is touched on the device again (a leak, on purpose)."""
        self.cos.clear()
        self.ix._h = None

    def close(self):
        for co in list(self.cos):
            self.destroy(co)
        self.ix.close()

    # ---- requests ----
    def query_terms(self, nt, n_segs=None, absent=0.15):
        """nt distinct terms as per-segment ids, SLG_NO_TERM where the term is absent from a segment (never the
        first term in segment 0)."""
        n_segs = self.ix.n_segs if n_segs is None else n_segs
        t = self.rng.choice(self.vocab, size=nt, replace=False).astype(np.uint32)
        tids = np.repeat(t[:, None], n_segs, axis=1)
        gone = self.rng.random(tids.shape) < absent
        if nt:
            gone[0, 0] = False
        tids[gone] = self.N.NO_TERM
        return tids, (self.rng.random(nt) * 2 + 0.25).astype(np.float32)

    def run(self, fns):
        """Run every fn on a daemon thread of its own; Hung if one does not come back."""
        errors = []

        def guard(fn):
            def body():
                try:
                    fn()
                except BaseException as e:  # noqa: BLE001 (reported on the test's thread)
                    errors.append(e)
            return body

        th = [threading.Thread(target=guard(f), daemon=True) for f in fns]
        for t in th:
            t.start()
        hung = False
        for t in th:
            t.join(0.0 if hung else BOUND)
            hung = hung or t.is_alive()
        if hung:
            self.abandon()
            raise Hung(f"a coalescer caller did not return within {BOUND:.0f} s")
        if errors:
            raise errors[0]

    # ---- the C ABI ----
    def search(self, co, row, k, strategy=None, want_stats=False):
        """slg_coalescer_search_plan -> (rc, doc, seg, score, count, stats, error text), outputs pre-filled."""
        N, lib = self.N, self.lib
        d, s = np.full(k, 0xABABABAB, np.uint32), np.full(k, 0xABABABAB, np.uint32)
        sc, c = np.full(k, np.float32(-7.0)), C.c_uint32(0xABABABAB)
        st = N.Stats()
        rc = lib.slg_coalescer_search_plan(co, C.addressof(row.query), None if row.leaf is None else row.leaf.ctypes.data,
                                           row.plan, row.tie, row.n_leaves, row.filter_id, k,
                                           self.sa.Wand if strategy is None else strategy, d.ctypes.data, s.ctypes.data,
                                           sc.ctypes.data, C.addressof(c), C.addressof(st) if want_stats else None)
        err = lib.slg_coalescer_last_error().decode()
        return rc, d, s, sc, c.value, st, err

    def submit(self, co, row, k, want_stats=0, strategy=None):
        t = self.N.Ticket()
        rc = self.lib.slg_coalescer_submit(co, C.addressof(row.query), None if row.leaf is None else row.leaf.ctypes.data,
                                           row.plan, row.tie, row.n_leaves, row.filter_id, k,
                                           self.sa.Wand if strategy is None else strategy, want_stats, C.addressof(t))
        return rc, t, self.lib.slg_coalescer_last_error().decode()

    def wait(self, co, ticket, k, stats=None):
        d, s = np.full(k, 0xABABABAB, np.uint32), np.full(k, 0xABABABAB, np.uint32)
        sc, c = np.full(k, np.float32(-7.0)), C.c_uint32(0xABABABAB)
        rc = self.lib.slg_coalescer_wait(co, C.addressof(ticket), d.ctypes.data, s.ctypes.data, sc.ctypes.data,
                                         C.addressof(c), None if stats is None else C.addressof(stats))
        return rc, d, s, sc, c.value, self.lib.slg_coalescer_last_error().decode()

    def counters(self, co):
        nb, nq = C.c_uint64(0), C.c_uint64(0)
        assert self.lib.slg_coalescer_stats(co, C.addressof(nb), C.addressof(nq)) == 0
        return nb.value, nq.value


def same_row(got, ref, i, what):
    """got = (doc, seg, score, count) of one request; ref = the reference arrays; row i of them."""
    d, s, sc, n = got
    rd, rs, rsc, rn = ref
    assert n == int(rn[i]), f"{what}: count {n}, reference {int(rn[i])}"
    assert np.array_equal(d[:n], rd[i, :n]) and np.array_equal(s[:n], rs[i, :n]), f"{what}: docs differ"
    assert np.array_equal(sc[:n].view(np.uint32), rsc[i, :n].view(np.uint32)), f"{what}: score bits differ"
    assert not d[n:].any() and not s[n:].any() and not sc[n:].view(np.uint32).any(), f"{what}: not zero past the count"


@pytest.fixture(scope="module")
def world(sa):
    W = World(sa, 2024)
    yield W
    W.close()


def planned_cases(W, nt):
    """Case (a): the shapes of a flat plan, for a query of nt >= 4 terms."""
    tids, w = W.query_terms(nt)
    base = Row(tids, w)
    pairs = np.arange(nt, dtype=np.uint32) // 2             # two terms in one leaf
    shuffled = W.rng.permutation(nt).astype(np.uint32)      # leaves named out of order
    return [
        ("sum, explicit leaves", base.variant(leaf=np.arange(nt), n_leaves=nt)),
        ("dismax tie 0", base.variant(leaf=np.arange(nt), plan=DISMAX, tie=0.0, n_leaves=nt)),
        ("dismax tie 0.3", base.variant(leaf=np.arange(nt), plan=DISMAX, tie=0.3, n_leaves=nt)),
        ("dismax tie 1", base.variant(leaf=np.arange(nt), plan=DISMAX, tie=1.0, n_leaves=nt)),
        ("two terms in one leaf, dismax", base.variant(leaf=pairs, plan=DISMAX, tie=0.3, n_leaves=int(pairs.max()) + 1)),
        ("two terms in one leaf, sum", base.variant(leaf=pairs, plan=SUM, n_leaves=int(pairs.max()) + 1)),
        ("leaves out of order", base.variant(leaf=shuffled // 2, plan=DISMAX, tie=0.3, n_leaves=int((shuffled // 2).max()) + 1)),
        ("derived leaf count", base.variant(leaf=shuffled // 2, plan=DISMAX, tie=0.3, n_leaves=0)),
        ("a leaf without terms", base.variant(leaf=pairs, plan=DISMAX, tie=0.3, n_leaves=int(pairs.max()) + 3)),
        ("leaf NULL, dismax", base.variant(leaf=None, plan=DISMAX, tie=0.3, n_leaves=0)),
    ]


@pytest.fixture(scope="module")
def alone_rows(world):
    named = []
    for nt in (4, 5, 6):
        for name, row in planned_cases(world, nt):
            for fname, f in (("no filter", -1), ("half filter", world.f_half), ("reject-all filter", world.f_none)):
                named.append((f"{name}, {nt} terms, {fname}", row.variant(filter_id=f)))
    return [n for n, _ in named], RowSet([r for _, r in named])


@pytest.mark.parametrize("k", [11, 300])
def test_planned_and_filtered_rows_alone(world, oracle, alone_rows, k):
    """(a) Every shape of a flat plan x {no filter, half filter, reject-all filter} through
    slg_coalescer_search_plan from one caller: the per-row plan and filter slots, the derived leaf count, the copy
    of the leaves into the batch; k = 11 (register top-k) and 300 (select path)."""
    names, rows = alone_rows
    ref = rows.reference(world, k, oracle)
    flat = RowSet([r.variant(leaf=None, plan=SUM, tie=0.0, n_leaves=0) for r in rows.rows]).batch(world, k)
    assert not np.array_equal(ref[2].view(np.uint32), flat[2].view(np.uint32))  # the plans matter
    assert int(ref[3][[i for i, r in enumerate(rows.rows) if r.filter_id == world.f_none]].sum()) == 0
    co = world.coalescer(64)
    out = [None] * len(rows.rows)

    def caller():
        for i, r in enumerate(rows.rows):
            out[i] = world.search(co, r, k)

    world.run([caller])
    world.destroy(co)
    for i, (rc, d, s, sc, n, _, err) in enumerate(out):
        assert rc == 0, f"{names[i]}: rc {rc} ({err})"
        same_row((d, s, sc, n), ref, i, names[i])


def mixed_rows(W, nq):
    """Case (b): per query, one row of each kind a request may draw."""
    rows, kinds = [], []
    for q in range(nq):
        nt = 1 + q % 6
        tids, w = W.query_terms(nt)
        plain = Row(tids, w)
        grouped = np.arange(nt, dtype=np.uint32) // 2
        for kind, row in (("plain", plain),
                          ("planned sum", plain.variant(leaf=grouped, n_leaves=0)),
                          ("dismax", plain.variant(leaf=W.rng.permutation(nt), plan=DISMAX, tie=0.3, n_leaves=nt + 1)),
                          ("filtered", plain.variant(filter_id=W.f_half if q % 5 else W.f_none)),
                          ("planned + filtered", plain.variant(leaf=grouped, plan=DISMAX, tie=1.0, n_leaves=0,
                                                               filter_id=W.f_half))):
            rows.append(row)
            kinds.append(kind)
    rows.append(Row(np.zeros((0, W.ix.n_segs), np.uint32), np.zeros(0, np.float32)))
    kinds.append("empty query")
    return kinds, RowSet(rows)


@pytest.fixture(scope="module")
def mixed(world, oracle):
    kinds, rows = mixed_rows(world, 64)
    rows.reference(world, 11, oracle)
    return kinds, rows


def concurrent(world, co, requests, k, n_threads=16, depth=8):
    """requests[i] = Row.  n_threads callers keep `depth` tickets in flight each (slg_coalescer_submit / _wait);
    -> per request (rc, doc, seg, score, count, error text), rc and text of the submit if that failed."""
    out = [None] * len(requests)

    def caller(t):
        def body():
            mine = list(range(t, len(requests), n_threads))
            pending = []
            for i in mine + [None] * depth:
                if i is not None:
                    rc, ticket, err = world.submit(co, requests[i], k)
                    if rc != 0:
                        out[i] = (rc, None, None, None, 0, err)
                    else:
                        pending.append((i, ticket))
                if pending and (i is None or len(pending) == depth):
                    j, ticket = pending.pop(0)
                    out[j] = world.wait(co, ticket, k)
        return body

    world.run([caller(t) for t in range(n_threads)])
    return out


@pytest.mark.parametrize("max_batch", [4, 1024])
def test_mixed_rows_share_batches(world, mixed, max_batch):
    """(b) 16 callers, 8 tickets in flight each, every request drawn from {plain, planned Sum, DisMax, filtered,
    planned + filtered, empty query}: rows with and without plans or filters share batches (any_plan / any_filter
    and the defaults a plain row gets in a planned batch), and every row is its reference row."""
    kinds, rows = mixed
    ref = rows.reference(world, 11)
    rng = np.random.default_rng(7 + max_batch)
    empty = len(rows.rows) - 1
    pick = [empty if rng.random() < 0.1 else int(rng.integers(0, empty)) for _ in range(640)]
    assert {kinds[i] for i in pick} == set(kinds)
    co = world.coalescer(max_batch)
    out = concurrent(world, co, [rows.rows[i] for i in pick], 11)
    n_batches, n_queries = world.counters(co)
    world.destroy(co)
    for i, (rc, d, s, sc, n, err) in zip(pick, out):
        assert rc == 0, f"{kinds[i]}: rc {rc} ({err})"
        same_row((d, s, sc, n), ref, i, kinds[i])
    assert n_queries == len(pick)
    assert n_batches < n_queries  # callers really shared batches: without it nothing here is about mixing


def faults(W, N):
    """Case (c): name -> (what it does to a good row, rc, words slg_coalescer_last_error must hold, whether the
    batch API refuses the same row).  Every row these are applied to has >= 2 terms, the first of them present
    in segment 0 with postings, so slg_batch_prepare_plan does refuse the non-finite weight there
    (slg_plan.cpp: build_subquery checks a weight once its term is known to have postings): the item stays."""
    n_terms = [s.n_terms for s in W.ix.segments]

    def leaf_2_31(r):
        leaf = np.arange(r.nt, dtype=np.uint32)
        leaf[-1] = 1 << 31
        return r.variant(leaf=leaf)

    def term(value):
        def f(r):
            tids = r.tids.copy()
            tids[0, 0] = value
            return r.variant(tids=tids)
        return f

    def weight(value):
        def f(r):
            w = r.w.copy()
            w[0] = value
            return r.variant(w=w)
        return f

    return {
        "tie -0.1": (lambda r: r.variant(tie=-0.1), N.ERR_INVALID, "tie breaker", True),
        "tie 1.5": (lambda r: r.variant(tie=1.5), N.ERR_INVALID, "tie breaker", True),
        "tie NaN": (lambda r: r.variant(tie=math.nan), N.ERR_INVALID, "tie breaker", True),
        "unknown plan": (lambda r: r.variant(plan=7), N.ERR_INVALID, "plan", True),
        "leaf 2^31": (leaf_2_31, N.ERR_INVALID, "leaf", True),
        "term id at the term count": (term(n_terms[0]), N.ERR_INVALID, "term id", True),
        "term id beyond the term count": (term(0xFFFFFFFE), N.ERR_INVALID, "term id", True),
        "filter never registered": (lambda r: r.variant(filter_id=57), N.ERR_INVALID, "filter", True),
        # (the batch API reads every negative id as "no filter"; the coalescer's header asks for -1)
        "negative filter id": (lambda r: r.variant(filter_id=-5), N.ERR_INVALID, "filter", False),
        "weight inf": (weight(math.inf), N.ERR_INVALID, "weight", True),
        "weight NaN": (weight(math.nan), N.ERR_INVALID, "weight", True),
    }


FAULTS = ["tie -0.1", "tie 1.5", "tie NaN", "unknown plan", "leaf 2^31", "term id at the term count",
          "term id beyond the term count", "filter never registered", "negative filter id", "weight inf", "weight NaN"]


@pytest.mark.parametrize("fault", FAULTS)
def test_bad_row_fails_only_its_caller(world, mixed, fault):
    """(c) The concurrent shape of (b) with exactly one fault in every seventh request.  The faulty request is
    refused — as slg_batch_prepare_plan refuses the same row on its own — with a text that names the cause;
    every other request gets its reference row; sharing happened."""
    N = world.N
    kinds, rows = mixed
    ref = rows.reference(world, 11)
    break_it, want_rc, words, batch_refuses = faults(world, N)[fault]
    good = [i for i, r in enumerate(rows.rows) if r.nt >= 2]
    rng = np.random.default_rng(len(fault) + 100 * FAULTS.index(fault))
    pick = [int(rng.integers(0, len(rows.rows))) for _ in range(448)]
    requests, bad = [], set()
    for j, i in enumerate(pick):
        if j % 7 == 3:
            i = pick[j] = good[int(rng.integers(0, len(good)))]
            requests.append(break_it(rows.rows[i]))
            bad.add(j)
        else:
            requests.append(rows.rows[i])
    one = RowSet([requests[min(bad)]])
    if batch_refuses:  # the batch API's verdict on the same row, alone
        with pytest.raises(world.sa.SlgError) as e:
            one.batch(world, 11)
        assert e.value.code == want_rc and words in e.value.msg, e.value
    else:
        one.batch(world, 11)
    co = world.coalescer(64)
    out = concurrent(world, co, requests, 11)
    n_batches, n_queries = world.counters(co)
    world.destroy(co)
    for j, (i, (rc, d, s, sc, n, err)) in enumerate(zip(pick, out)):
        if j in bad:
            assert rc == want_rc and words in err, f"faulty request {j}: rc {rc}, text {err!r}"
        else:
            assert rc == 0, f"good request {j} ({kinds[i]}): rc {rc} ({err})"
            same_row((d, s, sc, n), ref, i, kinds[i])
    assert n_queries == len(pick) - len(bad)
    assert n_batches < n_queries


def test_bad_k_and_strategy_take_no_kind(world, mixed):
    """k > SLG_MAX_K and an unknown strategy are refused before a kind is handed out: a coalescer that has
    refused more of them than it has kinds still serves eight combinations at once."""
    N = world.N
    _, rows = mixed
    row = rows.rows[5]
    co = world.coalescer(64)
    out = []

    def caller():
        for i in range(10):
            out.append(world.search(co, row, N.MAX_K + 1 + i)[::6])
            out.append(world.search(co, row, 11, strategy=3 + i)[::6])
        out.append(world.search(co, row, 11))

    world.run([caller])
    world.destroy(co)
    for j in range(0, 20, 2):
        assert out[j][0] == N.ERR_UNSUPPORTED and "SLG_MAX_K" in out[j][1], out[j]
        assert out[j + 1][0] == N.ERR_INVALID and "strategy" in out[j + 1][1], out[j + 1]
    rc, d, s, sc, n, _, err = out[-1]
    assert rc == 0, err
    same_row((d, s, sc, n), rows.reference(world, 11), 5, "after the refusals")


KS = [0, 1, 64, 65, 256, 257, 1024, 1025, 20001, 11, 300, 2000]


def test_kinds_are_reusable(world, oracle):
    """(d) Twelve k values one after the other on one coalescer (more than the eight kinds it collects at once),
    then the first again; then nine callers at once, each with a k of its own: the only refusal accepted is
    SLG_ERR_UNSUPPORTED "too many ... at once", and a refused caller succeeds once the others have returned."""
    N = world.N
    assert N.MAX_K in KS and len(set(KS)) == 12
    rows = RowSet([Row(*world.query_terms(nt)) for nt in (1, 2, 3, 6)] +
                  [Row(*world.query_terms(4)).variant(leaf=[1, 0, 1, 0], plan=DISMAX, tie=0.3, filter_id=world.f_half)])
    refs = {}
    for k in KS:
        if k:
            refs[k] = rows.reference(world, k, oracle)
        else:  # (query/wand.rs:413-416: k == 0 is no work; no arrays to compare)
            refs[k] = tuple(np.zeros((len(rows.rows), 0), t) for t in (np.uint32, np.uint32, np.float32)) + \
                (np.zeros(len(rows.rows), np.uint32),)
    co = world.coalescer(64)
    seq = []

    def one_after_the_other():
        for k in KS + [KS[0], KS[1]]:
            for i, r in enumerate(rows.rows):
                seq.append((k, i, world.search(co, r, k)))

    world.run([one_after_the_other])
    for k, i, (rc, d, s, sc, n, _, err) in seq:
        assert rc == 0, f"k={k}: rc {rc} ({err})"
        same_row((d, s, sc, n), refs[k], i, f"k={k}, row {i}")

    ks = KS[3:12]
    first = [None] * len(ks)
    gate = threading.Barrier(len(ks))

    def at_once(j):
        def body():
            gate.wait(BOUND)
            first[j] = world.search(co, rows.rows[j % len(rows.rows)], ks[j])
        return body

    world.run([at_once(j) for j in range(len(ks))])
    again = {}

    def retry():
        for j, r in enumerate(first):
            if r[0] != 0:
                again[j] = world.search(co, rows.rows[j % len(rows.rows)], ks[j])

    world.run([retry])
    world.destroy(co)
    for j, (rc, d, s, sc, n, _, err) in enumerate(first):
        if rc != 0:
            assert rc == N.ERR_UNSUPPORTED and "too many" in err and "at once" in err, f"k={ks[j]}: rc {rc} ({err})"
            rc, d, s, sc, n, _, err = again[j]
        assert rc == 0, f"k={ks[j]}: rc {rc} ({err})"
        same_row((d, s, sc, n), refs[ks[j]], j % len(rows.rows), f"k={ks[j]} at once")


def test_index_updates_under_a_live_coalescer(sa, oracle):
    """(e) add_segment / remove_segment / update_deleted between searches on one coalescer, nothing in flight
    during an update.  The segment count runs 2, 3, 4, 5, 6, 5, 4 with two k values: ten (k, segment count)
    combinations, more than collect at once.  Every search equals the batch API on the index as it then is (and,
    before the first update, the oracle); a filter registered before add_segment has no bitmap for the new
    segment, and the request that names it is refused at submit."""
    W = World(sa, 77, updatable=True)
    try:
        co = W.coalescer(64)
        shapes = [(1, None), (2, None), (3, "sum"), (4, "dismax"), (6, "dismax"), (5, None)]
        seen = set()

        def search_all(what, with_oracle=False, filters=True):
            rows = []
            for nt, plan in shapes:
                r = Row(*W.query_terms(nt))
                if plan:
                    r = r.variant(leaf=np.arange(nt) // 2, plan=DISMAX if plan == "dismax" else SUM, tie=0.3)
                rows.append(r)
                if filters:
                    rows.append(r.variant(filter_id=W.f_half))
            rs = RowSet(rows)
            for k in (11, 300):
                ref = rs.reference(W, k, oracle if with_oracle else None)
                out = []
                W.run([lambda: out.extend(W.search(co, r, k) for r in rows)])
                for i, (rc, d, s, sc, n, _, err) in enumerate(out):
                    assert rc == 0, f"{what}, k={k}, row {i}: rc {rc} ({err})"
                    same_row((d, s, sc, n), ref, i, f"{what}, k={k}, row {i}")
                seen.add((k, W.ix.n_segs))

        search_all("as created", with_oracle=True)
        for n in (3, 4, 5, 6):
            W.ix.add_segment(random_segment(W.rng, 300 + 50 * n, W.vocab, 25, k1=0.9, b=0.4))
            assert W.ix.n_segs == n
            search_all(f"{n} segments", filters=False)
        stale = []
        W.run([lambda: stale.append(W.search(co, Row(*W.query_terms(3)).variant(filter_id=W.f_half), 11))])
        assert stale[0][0] == W.N.ERR_INVALID and "filter" in stale[0][6], stale[0][::6]
        W.ix.remove_segment(1)   # the ordinals above it move down
        search_all("5 segments after a removal", filters=False)
        W.ix.remove_segment(3)
        search_all("4 segments after a removal", filters=False)
        assert len(seen) > 8
        seg = W.ix.segments[0]
        dead = np.zeros(seg.n_docs, bool)
        dead[::3] = True
        W.ix.update_deleted(0, np.packbits(dead, bitorder="little"), float(seg.n_docs - int(dead.sum())))
        search_all("after update_deleted", filters=False)
        W.destroy(co)
    finally:  # (after a hang the world is abandoned and this closes nothing)
        W.close()


def stats_tuple(st):
    return int(st.scored_docs), int(st.candidates_examined), int(st.postings_advanced)


def test_stats_present_absent_and_recycled(world, mixed):
    """(f) want_stats = 1: the request gets the slg_stats slg_batch_fetch reports for that query in the reference
    batch.  All three fields are per query (scored_docs = candidates_examined = docs that got a score,
    postings_advanced = postings of the query's lists) under SLG_STRATEGY_BM25, which is what is compared; under
    Wand / Bmw the header makes them depend on the pruning the batch ran with, so they are left out.
    want_stats = 0 afterwards, on the same kind, so that batch objects with earlier numbers are reused: a stats
    struct passed to slg_coalescer_wait comes back untouched, also for a ticket that may share its batch with one
    that did ask.

    Recycling after a FAILED batch is not tested: with every per-row refusal made at submit, the refusals left at
    batch level are device and memory errors and an index update or filter removal that races the collection, and
    none of them can be forced without a fault or a race."""
    N, sa = world.N, world.sa
    kinds, rows = mixed
    some = RowSet(rows.rows[3:43:6] + rows.rows[-1:])  # one of each kind a few times over, and the empty query
    full = some.batch(world, 11, strategy=sa.Bm25, want_stats=True)
    ref, ref_stats = full[:4], [stats_tuple(full[4][i]) for i in range(len(some.rows))]
    assert any(t[0] for t in ref_stats) and any(t[2] for t in ref_stats)
    co = world.coalescer(64)
    with_stats, without, paired = [], [], []

    def caller():
        for r in some.rows:
            with_stats.append(world.search(co, r, 11, strategy=sa.Bm25, want_stats=True))
        for r in some.rows:
            rc, t, err = world.submit(co, r, 11, want_stats=0, strategy=sa.Bm25)
            assert rc == 0, err
            st = N.Stats()
            C.memset(C.addressof(st), PATTERN, C.sizeof(st))
            without.append(world.wait(co, t, 11, stats=st) + (bytes(st),))
        for r in some.rows:  # two tickets at once, one asks
            rc1, t1, _ = world.submit(co, r, 11, want_stats=1, strategy=sa.Bm25)
            rc0, t0, _ = world.submit(co, r, 11, want_stats=0, strategy=sa.Bm25)
            assert rc1 == 0 and rc0 == 0
            s1, s0 = N.Stats(), N.Stats()
            C.memset(C.addressof(s0), PATTERN, C.sizeof(s0))
            w0 = world.wait(co, t0, 11, stats=s0)
            w1 = world.wait(co, t1, 11, stats=s1)
            paired.append((w1, stats_tuple(s1), w0, bytes(s0)))

    world.run([caller])
    world.destroy(co)
    untouched = bytes([PATTERN]) * C.sizeof(N.Stats)
    for i in range(len(some.rows)):
        rc, d, s, sc, n, st, err = with_stats[i]
        assert rc == 0, err
        same_row((d, s, sc, n), ref, i, "with stats")
        assert stats_tuple(st) == ref_stats[i], f"row {i}"
        rc, d, s, sc, n, err, raw = without[i]
        assert rc == 0, err
        same_row((d, s, sc, n), ref, i, "without stats")
        assert raw == untouched, f"row {i}: a ticket submitted with want_stats = 0 had its stats written"
        w1, st1, w0, raw0 = paired[i]
        assert w1[0] == 0 and w0[0] == 0
        same_row(w1[1:5], ref, i, "paired, with stats")
        same_row(w0[1:5], ref, i, "paired, without stats")
        assert st1 == ref_stats[i] and raw0 == untouched, f"row {i}"


def test_ticket_misuse(world, mixed):
    """A ticket is good for one wait; poll of a waited ticket, and submit with a NULL coalescer, query or ticket,
    are SLG_ERR_INVALID with a text in slg_coalescer_last_error."""
    N, lib = world.N, world.lib
    _, rows = mixed
    row = rows.rows[7]
    co = world.coalescer(64)
    seen = {}

    def caller():
        rc, t, err = world.submit(co, row, 11)
        assert rc == 0, err
        while lib.slg_coalescer_poll(co, C.addressof(t)) == 0:
            pass
        assert lib.slg_coalescer_poll(co, C.addressof(t)) == 1
        seen["first"] = world.wait(co, t, 11)
        seen["ticket cleared"] = not t.batch
        seen["poll"] = lib.slg_coalescer_poll(co, C.addressof(t))
        seen["second"] = world.wait(co, t, 11)
        t2 = N.Ticket()
        args = (None, SUM, 0.0, 0, -1, 11, world.sa.Wand, 0)
        for what, a, q, tk in (("coalescer", None, C.addressof(row.query), C.addressof(t2)),
                               ("query", co, None, C.addressof(t2)), ("ticket", co, C.addressof(row.query), None)):
            seen[what] = (lib.slg_coalescer_submit(a, q, *args, tk), lib.slg_coalescer_last_error().decode())
        seen["after"] = world.search(co, row, 11)

    world.run([caller])
    world.destroy(co)
    ref = rows.reference(world, 11)
    assert seen["first"][0] == 0 and seen["ticket cleared"]
    same_row(seen["first"][1:5], ref, 7, "first wait")
    assert seen["poll"] == N.ERR_INVALID
    assert seen["second"][0] == N.ERR_INVALID and seen["second"][5]
    for what in ("coalescer", "query", "ticket"):
        assert seen[what][0] == N.ERR_INVALID and "NULL" in seen[what][1], (what, seen[what])
    assert seen["after"][0] == 0
    same_row(seen["after"][1:5], ref, 7, "after the misuse")
