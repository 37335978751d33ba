"""The worlds of the many-term scoring kernel's edge tests: plain data, no device (test infrastructure).

tests/test_gpu_multi_edges.py runs them on the device; tests/test_multi_worlds.py proves on the CPU, through the
planner and tests/multi_model.py, that each world reaches the edges it promises (World.edges).

Every list is explicit.  A world is laid out round by round: the planner splits a sub-query at every `stride`-th
posting of its longest essential list (the splitter), so a world gives the splitter exactly `stride` postings per
round, the first of them the round's lowest doc, and places the other lists' postings of the round behind it.  The
number of rounds follows from the posting counts and the tuning (slg_plan.cpp plan_rounds): `multi_round_target` is
chosen as ceil(essential postings / rounds), and n_docs is kept small enough that the planner's density rule
(0.85 * 16 384 * postings / n_docs) does not lower it.  The CPU test asserts the rounds the planner really makes.

MaxScore worlds (strategies Wand / Bmw): one heavily weighted essential list of a few postings and long, lightly
weighted lists.  A list is block-skipped only if it is longer than 32 times the essential postings, and the threshold
seed of rank k is zero unless the essential list has k postings, so with lists of a few thousand postings the
classified edges exist at k = 1 alone (World.edge_ks); at the other k the batch is classified differently or not at
all, and the model predicts the run the planner then makes."""
import numpy as np

NO_TERM = 0xFFFFFFFF
BM25, WAND, BMW = 0, 1, 2
ALL_KS = (1, 64, 65, 256, 257)
PLAN_SUM, PLAN_DISMAX, PLAN_LEAF = 0, 1, 2


def segment(n_docs, lists, seed=1):
    """a one-field segment over explicit lists; tf from a fixed pattern, random doc lengths"""
    from searchlite_amd.segment import Segment
    offs, docs, tfs = [0], [], []
    for d in lists:
        d = np.asarray(d, dtype=np.int64)
        assert len(d) and (np.diff(d) > 0).all() and d[0] >= 0 and d[-1] < n_docs, "lists are ascending and inside the segment"
        docs.append(d.astype(np.uint32))
        tfs.append((d % 5 + 1).astype(np.uint32))
        offs.append(offs[-1] + len(d))
    dl = np.random.default_rng(seed).integers(5, 60, size=n_docs).astype(np.float32)
    return Segment(n_docs=n_docs, term_offsets=np.array(offs, dtype=np.uint64), doc_ids=np.concatenate(docs),
                   tfs=np.concatenate(tfs), field_doc_len=[dl], field_avgdl=[float(dl.mean())], docs=float(n_docs),
                   k1=1.2, b=0.75)


def by_rounds(T, rounds):
    """rounds: per round {list: docs} -> the T lists"""
    return [np.concatenate([np.asarray(r.get(t, []), dtype=np.int64) for r in rounds]) for t in range(T)]


def ar(lo, n, step=1):
    return lo + np.arange(n, dtype=np.int64) * step


def spread(lo, hi, n, phase=0):
    """n distinct docs over [lo, hi), evenly; lists with different phases do not share docs while phase < step"""
    step = (hi - lo) // n
    return lo + phase + np.arange(n, dtype=np.int64) * step


class World:
    def __init__(self, name, segs, terms, w, tuning, edges, strategies=(BM25,), edge_ks=ALL_KS, plans=None, nq=1,
                 n_rounds=None, always_multi=True):
        self.name, self.segs, self.tuning, self.plans = name, segs, dict(tuning), plans
        terms = np.asarray(terms, dtype=np.uint32)
        self.terms = terms.reshape(-1, len(segs))
        T = len(self.terms) // nq
        self.offs = (np.arange(nq + 1) * T).astype(np.uint32)
        self.w = np.asarray(w, dtype=np.float32)
        assert len(self.w) == len(self.terms)
        self.edges = edges            # {strategy: [edge names]} promised at every k of edge_ks
        self.strategies = tuple(strategies)
        self.edge_ks = tuple(edge_ks)
        self.n_rounds = n_rounds      # per segment, of query 0 (asserted by the CPU test where given)
        # False: 5..8 lists under the default tuning, on the many-term kernel only where the batch is classified
        self.always_multi = always_multi

    def __repr__(self):
        return self.name


def _target(ess, nr):
    t = -(-ess // nr)
    assert 64 <= t <= 512 and -(-ess // t) == nr, (ess, nr, t)
    return t


def _dense_enough(n_docs, ess, target):
    assert 0.85 * 16384 * ess / n_docs >= target, "the planner's density rule would lower the round target"


_worlds = {}


def _cached(fn):
    def get():
        if fn.__name__ not in _worlds:
            _worlds[fn.__name__] = fn()
        return _worlds[fn.__name__]
    get.__name__ = fn.__name__
    get.__doc__ = fn.__doc__
    return get


@_cached
def acc_world():
    """Accumulator edges, Bm25, T = 9, the splitter is list 4 with 64 postings per round (7 rounds of 1 000 docs, two
    rounds per slice: 4 slices, the last of one round).
      round 0: 512 postings on 512 distinct docs (rank 511 is used, no cut); list 0 has 65 postings
      round 1: 513 postings: list 0 has one (its share truncates to 0 and is clamped to 1: taken whole), the others 64
               each: cut inside their slot
      round 2: 1 488 postings: four chunks
      rounds 3, 4, 5: the first, a middle, the last list without a posting (the slot owner clamp)
      round 6: a small round"""
    T, nr, stride = 9, 7, 64
    rounds = []
    for r in range(nr):
        base = 1000 * r
        rd = {4: ar(base, stride, 15)}
        others = [t for t in range(T) if t != 4]
        if r == 0:
            sizes = dict(zip(others, [65, 55, 55, 55, 55, 55, 54, 54]))
        elif r == 1:
            sizes = dict(zip(others, [1] + [64] * 7))
        elif r == 2:
            sizes = dict(zip(others, [178] * 8))
        else:
            sizes = dict(zip(others, [9, 11, 13, 8, 12, 10, 7, 14]))
            sizes.pop({3: 0, 4: 3, 5: 8}.get(r, -1), None)
        for j, t in enumerate(others):
            if t in sizes:   # residues 1..8 of 15 (r == 2: of 5): no doc is shared with the splitter
                rd[t] = ar(base + 1 + j % 4, sizes[t], 5) if r == 2 else ar(base + 1 + j, sizes[t], 15)
        rounds.append(rd)
    lists = by_rounds(T, rounds)
    ess = sum(len(x) for x in lists)
    n_docs = 8000
    mrt = _target(ess, nr)
    _dense_enough(n_docs, ess, mrt)
    edges = ["R_ess==512 uncut, 512 docs", "R_ess==513 cut, a list clamped to 1, a list cut inside a slot",
             "a cut round of >= 3 chunks", "a list with 64 postings in a round", "a list with 65 postings in a round",
             "first list empty in a round", "middle list empty in a round", "last list empty in a round", "T==9",
             "n_rounds not a multiple of rounds_per_slice", ">= 3 slices"]
    return World("acc", [segment(n_docs, lists)], np.arange(T), 0.5 + np.arange(T) * 0.25,
                 dict(multi_round_target=mrt, rounds_per_slice=2), {BM25: edges}, n_rounds=[nr])


@_cached
def slots_world():
    """Slot and batch edges, Bm25, T = 12, the splitter is list 0 with 53 postings per round (4 rounds of 2 000 docs):
    rounds of 8, 9, 16 and 17 slots = 1, 2, 2 and 3 batches of sweep A."""
    T, nr, stride = 12, 4, 53
    per_round = [  # postings of lists 1..11
        [40, 3, 20, 9, 5, 7, 30, 0, 0, 0, 0],          # 8 slots
        [40, 3, 20, 9, 5, 7, 30, 2, 0, 0, 0],          # 9 slots
        [65, 65, 65, 65, 65, 1, 1, 1, 1, 1, 0],         # 1 + 10 + 5 = 16 slots
        [65, 65, 65, 65, 65, 1, 1, 1, 1, 1, 1],         # 17 slots
    ]
    rounds = []
    for r in range(nr):
        base = 2000 * r
        rd = {0: ar(base, stride, 37)}
        for j, n in enumerate(per_round[r]):
            if n:
                rd[j + 1] = ar(base + 1 + j, n, 13)
        rounds.append(rd)
    lists = by_rounds(T, rounds)
    assert len(lists[0]) > max(len(x) for x in lists[1:])
    ess = sum(len(x) for x in lists)
    n_docs = 8000
    mrt = _target(ess, nr)
    _dense_enough(n_docs, ess, mrt)
    edges = ["S==8", "S==9", "S==16", "S==17", "nb_a==1", "nb_a==2", "nb_a==3"]
    return World("slots", [segment(n_docs, lists)], np.arange(T), 0.5 + np.arange(T) * 0.125,
                 dict(multi_round_target=mrt, rounds_per_slice=3), {BM25: edges}, n_rounds=[nr])


@_cached
def t32_world():
    """T = 32 with one posting per list: one round of 32 slots = 4 batches of sweep A; every third doc is shared by
    two lists."""
    T = 32
    lists = [np.array([10 + 3 * (t - t % 3 // 2)]) for t in range(T)]
    edges = ["T==32, one posting per list", "nb_a==4", "T==32"]
    return World("t32", [segment(500, lists)], np.arange(T), 0.25 + np.arange(T) * 0.0625, {}, {BM25: edges},
                 n_rounds=[1])


@_cached
def window_world():
    """Window edges, Bm25, T = 9, the splitter is list 0 with 8 postings per round, 64 postings per round (the planner's
    floor for sparse lists), 10 rounds.  B = 32 * 40:
      round 0: docs [B, B + 16 384): the window exactly, docs at its bits 0, 31, 32 and 16 383; no cut
      round 1: docs [B + 16 384, B + 32 769): one doc too many: a window cut, and a second chunk of one doc
      round 2: starts at B + 32 769 (not a multiple of 32) and spans 16 384 docs: from its window base it is 16 385
      round 3: docs near its start, then more than five empty windows, then the rest
      rounds 4..9: 300 docs each"""
    T, nr, stride = 9, 10, 8
    B = 32 * 40
    starts = [B, B + 16384, B + 32769, B + 32769 + 16384]
    starts.append(starts[3] + 7 * 16384)
    for r in range(5, nr + 1):
        starts.append(starts[-1] + 300)
    rounds = []
    for r in range(nr):
        lo, hi = starts[r], starts[r + 1]
        rd = {}
        if r < 3:
            rd[0] = np.concatenate([[lo], spread(lo + 100, hi - 100, stride - 1)])
            for t in range(1, T):
                rd[t] = spread(lo + 40, hi - 40, 7, phase=t)
            rd[1] = np.concatenate([[lo], rd[1][1:]])               # bit 0 (r == 0) twice
            rd[2] = np.concatenate([[lo + 31, lo + 32], rd[2][2:]])
            rd[3] = np.concatenate([rd[3][:-1], [hi - 1]])           # the round's last doc
            if r == 2:
                rd[4] = np.concatenate([rd[4][:-1], [lo - lo % 32 + 16383]])   # the last doc of the cut window
        elif r == 3:
            rd[0] = np.concatenate([[lo], spread(lo + 50, lo + 2000, 3), spread(hi - 3000, hi - 10, 4)])
            for t in range(1, T):
                rd[t] = np.concatenate([spread(lo + 10, lo + 3000, 3, phase=t), spread(hi - 4000, hi - 100, 4, phase=t)])
        else:
            rd[0] = ar(lo, stride, 30)
            for t in range(1, T):
                rd[t] = ar(lo + t, 7, 37)
        rounds.append(rd)
    lists = by_rounds(T, rounds)
    ess = sum(len(x) for x in lists)
    assert ess == 64 * nr
    n_docs = starts[-1] + 100
    edges = ["dhi-wbase==16384 uncut", "dhi-wbase==16385", "rdhi-dlo<=16384 but dlo%32!=0 cuts",
             "docs at window bits 0, 31, 32, 16383", "next chunk several empty windows on", "ndocs==1"]
    return World("window", [segment(n_docs, lists)], np.arange(T), 0.5 + np.arange(T) * 0.25,
                 dict(multi_round_target=64, rounds_per_slice=4), {BM25: edges}, n_rounds=[nr])


def _plan_lists():
    """The lists of the three plan worlds: T = 9, the splitter is list 4 with 128 postings per round, 4 rounds.
    Round 0 spans docs [0, 30 000) with 552 postings: a proportional cut, whose chunk still spans more than the window;
    lists 5 and 6 have one posting in the round, in its first window, so they are idle in its second chunk."""
    T, nr, stride = 9, 4, 128
    rounds = []
    for r in range(nr):
        rd = {}
        if r == 0:
            rd[4] = spread(0, 30000, stride)
            for j, t in enumerate([0, 1, 2, 3, 5, 6, 7, 8]):
                rd[t] = spread(5, 29990, 70, phase=j * 3)
                if t in (5, 6):   # one posting: taken whole by the proportional cut, and gone after the first chunk
                    rd[t] = rd[t][20:21]
            rd[8] = np.concatenate([rd[8], [rd[0][-1], rd[4][-1]]])   # docs shared with a positive leaf and alone
            rd[8] = np.unique(rd[8])
        else:
            lo = 30000 + 2000 * (r - 1)
            rd[4] = ar(lo, stride, 15)
            for j, t in enumerate([0, 1, 2, 3, 5, 6, 7, 8]):
                rd[t] = ar(lo + 15 * j, 10, 45) if (j + r) % 3 else ar(lo + 1 + j, 10, 45)
        rounds.append(rd)
    lists = by_rounds(T, rounds)
    ess = sum(len(x) for x in lists)
    n_docs = 36500
    mrt = _target(ess, nr)
    _dense_enough(n_docs, ess, mrt)
    return segment(n_docs, lists), mrt, nr


_PLAN_EDGES = ["a chunk cut by the accumulator rule and the window", "a negative weight",
               "an idle leaf in a round's later chunk"]
_PLAN_W = [1.0, 0.5, 2.0, 0.75, 1.5, 1.25, 0.5, 1.0, -0.5]
_PLAN_LEAF = [0, 0, 1, 2, 2, 3, 4, 5, 5]     # lists 5 and 6 = leaves 3 and 4


@_cached
def cut_both_world():
    """MODE 0 over the plan worlds' lists (no plan, positive weights): the proportional and the window cut in one
    chunk."""
    seg, mrt, nr = _plan_lists()
    return World("cut_both", [seg], np.arange(9), [abs(x) for x in _PLAN_W], dict(multi_round_target=mrt, rounds_per_slice=3),
                 {BM25: _PLAN_EDGES[:1]}, n_rounds=[nr])


@_cached
def plan_flat_world():
    """MODE 2: query 0 a flat Sum of 6 leaves, query 1 a DisMax (tie 0.4) of them; list 8 (leaf 5) weighs -0.5."""
    seg, mrt, nr = _plan_lists()
    plans = dict(q_leaf=np.array(_PLAN_LEAF * 2, np.uint32), q_plan=np.array([PLAN_SUM, PLAN_DISMAX], np.int32),
                 q_tie=np.array([0.0, 0.4], np.float32), q_nleaves=np.array([6, 6], np.uint32))
    return World("plan_flat", [seg], np.tile(np.arange(9), 2), _PLAN_W * 2, dict(multi_round_target=mrt, rounds_per_slice=3),
                 {BM25: _PLAN_EDGES + ["MODE 2"]}, plans=plans, nq=2, n_rounds=[nr])


@_cached
def plan_groups_world():
    """MODE 3: groups of leaves {0, 1, 2} (DisMax, tie 0.5), {3, 4} (DisMax, tie 0.25: idle in round 0's later chunks)
    and {5} (Sum); the root a Sum (query 0) or a DisMax with tie 0.25 (query 1)."""
    seg, mrt, nr = _plan_lists()
    plans = dict(q_leaf=np.array(_PLAN_LEAF * 2, np.uint32), q_plan=np.array([PLAN_SUM, PLAN_DISMAX], np.int32),
                 q_tie=np.array([0.0, 0.25], np.float32), q_nleaves=np.array([6, 6], np.uint32),
                 q_leaf_offsets=np.array([0, 6, 12], np.uint32), leaf_group=np.array([0, 0, 0, 1, 1, 2] * 2, np.uint32),
                 q_group_offsets=np.array([0, 3, 6], np.uint32),
                 group_plan=np.array([PLAN_DISMAX, PLAN_DISMAX, PLAN_SUM] * 2, np.int32),
                 group_tie=np.array([0.5, 0.25, 0.0] * 2, np.float32))
    return World("plan_groups", [seg], np.tile(np.arange(9), 2), _PLAN_W * 2,
                 dict(multi_round_target=mrt, rounds_per_slice=3), {BM25: _PLAN_EDGES + ["MODE 3", "an idle group"]},
                 plans=plans, nq=2, n_rounds=[nr])


@_cached
def plan_deep_world():
    """MODE 4: a tree of four internal levels (SLG_MAX_PLAN_DEPTH) with a leaf hanging off every level; the innermost
    Sum node holds leaves 3 and 4: idle in round 0's later chunks."""
    seg, mrt, nr = _plan_lists()
    S, D, L = PLAN_SUM, PLAN_DISMAX, PLAN_LEAF
    plans = dict(q_leaf=np.array(_PLAN_LEAF, np.uint32), q_node_offsets=np.array([0, 10], np.uint32),
                 node_kind=np.array([D, L, S, L, D, L, S, L, L, L], np.int32),
                 node_tie=np.array([.25, 0, 0, 0, .75, 0, 0, 0, 0, 0], np.float32),
                 node_parent=np.array([0, 0, 0, 2, 2, 4, 4, 6, 6, 0], np.uint32))
    return World("plan_deep", [seg], np.arange(9), _PLAN_W, dict(multi_round_target=mrt, rounds_per_slice=3),
                 {BM25: _PLAN_EDGES + ["MODE 4", "an idle node"]}, plans=plans, n_rounds=[nr])


@_cached
def two_segments_world():
    """Two segments, T = 9 in segment 0; list 3 does not exist in segment 1 (NO_TERM) and the lists there are other
    docs."""
    lists0 = [ar(3 + t, 40 + t, 17) for t in range(9)]
    lists1 = [ar(1 + 2 * t, 30 + 3 * t, 11) for t in range(8)]
    terms = [[t, NO_TERM if t == 3 else t - (t > 3)] for t in range(9)]
    return World("two_segments", [segment(900, lists0), segment(800, lists1, seed=2)], terms, 0.5 + np.arange(9) * 0.25,
                 {}, {BM25: ["two segments, a term absent from one"]})


MS_W_ESS, MS_W_REST = 1000.0, 0.01


def _ms_probe(name, tuning, always_multi):
    """MaxScore and block skipping, Wand / Bmw at k = 1, T = 5: list 2 is essential (8 postings, weight 1 000: the
    splitter, 2 postings per round), lists 0, 1, 3 and 4 are probed and block-skipped.  probe_target 512 makes 4 rounds.
    W = 32 * 100:
      round 0: docs [W, W + 16 384), essential docs at window bits 0 and 16 383.  List 0: a slot whose only hit is its
               first doc (bit 0), a slot without a hit (skipped, among the first 8), a slot whose only hit is its last
               doc (the window's last).  Lists 1, 3 and 4: slots without a hit, among the first 8 and behind them
      round 1: docs [W + 16 384, W + 40 000): a window cut.  List 0: a whole slot without a hit below the cut (skipped
               under a cut), a slot that straddles the cut, a slot past it; the second chunk has no essential posting
      round 2: 10 slots, the only skipped ones behind the first 8: one batch less
      round 3: the rest"""
    T = 5
    W = 3200
    r0, r1, r2, r3, end = W, W + 16384, W + 40000, W + 50000, W + 60000
    E = [np.array([r0, r0 + 16383]), np.array([r1, r1 + 5000]), np.array([r2, r2 + 9000]), np.array([r3, r3 + 9000])]
    rounds = []
    # round 0
    rounds.append({2: E[0],
                   0: np.concatenate([ar(r0, 64, 3), ar(r0 + 1000, 64, 3), ar(r0 + 16383 - 63 * 2, 64, 2)]),
                   1: np.concatenate([ar(r0 + 2, 64, 5), ar(r0 + 5000, 64, 5), ar(r0 + 9000, 30, 5)]),
                   3: ar(r0 + 7, 150, 11), 4: ar(r0 + 9, 160, 13)})
    # round 1: window base r1, the cut at r1 + 16 384
    cutdoc = r1 + 16384
    rounds.append({2: E[1],
                   0: np.concatenate([ar(r1 + 6000, 64, 2), ar(cutdoc - 40, 64, 2), ar(cutdoc + 500, 64, 2)]),
                   1: np.concatenate([ar(r1, 20, 250), ar(cutdoc + 10, 100, 7)]),
                   3: ar(r1 + 1, 128, 150), 4: ar(r1 + 4999, 70, 1)})
    # round 2: 10 slots; lists 0, 1 and 3 and the first slot of list 4 hit an essential doc (slots 0..7: kept), the
    # last two slots of list 4 do not
    rounds.append({2: E[2],
                   0: np.concatenate([ar(r2, 64, 10), ar(r2 + 8500, 60, 10)]),
                   1: np.concatenate([ar(r2, 64, 9), ar(r2 + 9000 - 63 * 9, 64, 9)]),
                   3: np.concatenate([ar(r2, 64, 7), ar(r2 + 9000 - 63 * 4, 64, 4)]),
                   4: np.concatenate([ar(r2, 64, 3), ar(r2 + 1001, 64, 9), ar(r2 + 9001, 64, 9)])})
    rounds.append({2: E[3], 0: ar(r3 + 1, 40, 9), 1: ar(r3, 130, 70), 3: ar(r3 + 2, 70, 100), 4: ar(r3 + 8990, 50, 5)})
    lists = by_rounds(T, rounds)
    total = sum(len(x) for x in lists)
    assert 512 * 3 < total <= 512 * 4 and min(len(lists[t]) for t in (0, 1, 3, 4)) > 32 * 8
    w = [MS_W_REST, MS_W_REST * 2, MS_W_ESS, MS_W_REST, MS_W_REST * 3]
    edges = ["T==5 classified", "a probed slot past the cut", "a whole probed slot with 0 hits",
             "a whole slot whose only hit is its first doc, at a bit with x&31==0",
             "a whole slot whose only hit is its last doc, the window's last", "a straddling slot is kept",
             "a skipped slot among the first 8", "skipped slots only behind the first 8", "nb drops",
             "a skipped whole slot under a cut", "a non-essential list before the essential one, docs present and absent",
             "no essential posting left in a round"]
    return World(name, [segment(end + 100, lists)], np.arange(T), w, dict(tuning, probe_target=512, rounds_per_slice=3),
                 {WAND: edges, BMW: edges}, strategies=(WAND, BMW), edge_ks=(1,), n_rounds=[4], always_multi=always_multi)


@_cached
def ms_probe_world():
    """_ms_probe under the default kernel choice: 5 lists run on the many-term kernel because they are classified and
    block skipping is expected to leave more than 15 % of the postings unread (k = 1); at the other k, and under Bm25,
    the batch is unclassified and runs on the few-term kernel."""
    return _ms_probe("ms_probe", {}, False)


@_cached
def ms_probe_multi_world():
    """_ms_probe with uniform_max_terms 4: 5 lists run on the many-term kernel at every k and strategy (MODE 0 where
    unclassified)."""
    return _ms_probe("ms_probe_multi", dict(uniform_max_terms=4), True)


@_cached
def ms_slots_world():
    """The slot rule, Wand / Bmw at k = 1, T = 32: list 31 is essential (4 postings, weight 1 000), the others are
    probed.  probe_target 2 100 makes 2 rounds:
      round 0: 30 lists of 65 postings + one of 10: 62 slots and 1 962 postings <= (63 - 32) * 64: the chunk is marked
               cut with a share of 1, and nothing is cut off
      round 1: 31 lists of 70 postings: 63 slots, 2 172 postings: the slot rule alone lowers the share"""
    T = 32
    r0, r1, end = 100, 6000, 12000
    # the essential docs: the round's first doc, and a doc of list 5 (round 0) / list 7 (round 1); in round 1 list 0
    # starts on the essential doc
    rounds = [{31: np.array([r0, r0 + 1 + 5 + 40 * 3])}, {31: np.array([r1, r1 + 7 + 40 * 30])}]
    for t in range(31):
        rounds[0][t] = ar(r0 + 1 + t, 65 if t < 30 else 10, 40)
        rounds[1][t] = ar(r1 + t, 70, 40)
    lists = by_rounds(T, rounds)
    total = sum(len(x) for x in lists)
    assert 2100 < total <= 4200
    w = [MS_W_REST * (1 + t % 3) for t in range(31)] + [MS_W_ESS]
    edges = ["S_all in 61..63 with share>=1: marked cut, nothing cut off", "the slot rule alone lowers share", "T==32"]
    return World("ms_slots", [segment(end, lists)], np.arange(T), w, dict(probe_target=2100, rounds_per_slice=1),
                 {WAND: edges, BMW: edges}, strategies=(WAND, BMW), edge_ks=(1,), n_rounds=[2])


WORLDS = (acc_world, slots_world, t32_world, window_world, cut_both_world, plan_flat_world, plan_groups_world, plan_deep_world,
          two_segments_world, ms_probe_world, ms_probe_multi_world, ms_slots_world)
