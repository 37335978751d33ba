"""The worlds of the few-term scoring kernel's edge tests: plain data, no device (test infrastructure).

tests/test_gpu_fewterm_edges.py runs them on the device; tests/test_fewterm_worlds.py proves on the CPU, through the
planner and tests/fewterm_model.py, that each world reaches the edges it promises (World.edges).

Every list is explicit and laid out round by round, as in tests/multi_worlds.py: the planner cuts a sub-query at every
`stride`-th posting of its longest list, so a world gives that list exactly `stride` postings per round, the first of
them the round's lowest doc, and places the other lists' postings behind it.  The number of rounds is
ceil(postings / uniform_round_target): a world picks the target that gives the rounds it was laid out for (the planner
clamps it to 48..512) and pins rounds_per_slice; the CPU test asserts the rounds and slices the planner really makes.
`pruning` is off in every world, so Wand runs unclassified on the few-term kernel too.

Unshared postings sit at doc = base + 16 i + 1 + list (the longest list at base + 16 i): lists never share a doc, nor a
filter field (8 192 and 4 096 are multiples of 16), unless a world says so."""
import numpy as np

from tests.multi_worlds import ALL_KS, BM25, NO_TERM, PLAN_DISMAX, PLAN_SUM, WAND, _cached, ar, segment

FULL_K_CAP = 1025


class World:
    """name, segments, queries (each a list of (per-segment term ids, weight)), tuning, strategies, the promised edges
    and the k values that matter beside ALL_KS; marks: docs the edge predicates look for"""

    def __init__(self, name, segs, queries, tuning, edges, ml, strategies=(BM25,), ks=(), plans=None, marks=None,
                 masks=None, n_rounds=None, n_slices=None):
        self.name, self.segs, self.plans = name, segs, plans
        self.tuning = dict(dict(pruning=0), **tuning)
        rows, w, offs = [], [], [0]
        for q in queries:
            for ids, weight in q:
                ids = [ids] * len(segs) if np.isscalar(ids) else list(ids)
                rows.append(ids)
                w.append(weight)
            offs.append(len(rows))
        self.terms = np.asarray(rows, dtype=np.uint32).reshape(-1, len(segs))
        self.offs = np.asarray(offs, dtype=np.uint32)
        self.w = np.asarray(w, dtype=np.float32)
        self.nq = len(queries)
        self.edges, self.ml = list(edges), ml          # ml: 4 or 8, the kernel instance the batch runs on
        self.strategies = tuple(strategies)
        self.ks = tuple(sorted(set(ALL_KS) | set(ks) | {self.full_k()}))
        self.marks = marks or {}
        self.masks = masks                             # a doc filter on every query: per segment a boolean pass mask
        self.n_rounds, self.n_slices = n_rounds, n_slices   # per sub-query, asserted by the CPU test where given

    def query_lists(self, q, s):
        from tests.fewterm_model import lists_of
        ids = [int(t) for t in self.terms[int(self.offs[q]):int(self.offs[q + 1]), s] if t != NO_TERM]
        return lists_of(self.segs[s], ids)

    def distinct_docs(self):
        return [sum(len(np.unique(np.concatenate(self.query_lists(q, s)))) for s in range(len(self.segs)))
                for q in range(self.nq)]

    def full_k(self):
        """a k that shows every doc of every query: its exact score is compared, not only the best ones"""
        return min(max(max(self.distinct_docs()), 1), FULL_K_CAP)

    def __repr__(self):
        return self.name


def fill(base, t, n, gap=1, skip=0):
    """n unshared docs of list t (0: the longest list) from base on"""
    return base + 16 * gap * (skip + np.arange(n, dtype=np.int64)) + (0 if t == 0 else 1 + t)


def merged(*parts):
    d = np.concatenate([np.asarray(p, dtype=np.int64).ravel() for p in parts])
    out = np.unique(d)
    assert len(out) == len(d), "a list holds a doc twice"
    return out


def by_rounds(T, rounds):
    lists = [merged(*[r.get(t, []) for r in rounds]) for t in range(T)]
    for r, nxt in zip(rounds, rounds[1:]):
        lo = min(int(np.min(v)) for v in nxt.values() if len(v))
        assert int(np.min(nxt[0])) == lo and all(int(np.max(v)) < lo for v in r.values() if len(v)), "rounds overlap"
    return lists


def target_for(lists, nr):
    """the uniform_round_target under which the planner makes nr rounds of these lists"""
    P = sum(len(x) for x in lists)
    t = max(48, -(-P // nr))
    assert t <= 512 and -(-P // t) == nr, (P, nr, t)
    assert all(len(lists[0]) > len(x) for x in lists[1:]), "list 0 is the longest"
    return t


def regular(T, nr, stride, counts, span, at_base=()):
    """nr rounds of `span` docs; list 0 has `stride` postings in each, list t counts[t - 1] (a number, or per round);
    at_base: rounds whose first doc sits in every list (it replaces each list's first posting of the round)"""
    rounds = []
    for r in range(nr):
        base = span * r
        rd = {0: fill(base, 0, stride, gap=max(1, (span // 16 - 1) // stride))}
        for t in range(1, T):
            c = counts[t - 1]
            c = c if np.isscalar(c) else c[r]
            if c:
                d = fill(base, t, c, gap=max(1, (span // 16 - 1) // c))
                if r in at_base:
                    d[0] = base
                rd[t] = d
        rounds.append(rd)
    return by_rounds(T, rounds)


def _ids(first, T):
    return [(first + t, 0.5 + 0.25 * t) for t in range(T)]


# ---- cuts ------------------------------------------------------------------------------------------------------
@_cached
def cuts4_world():
    """Cut edges on the 64-word row (4-bit instance), rounds of 1 500 docs and 48 postings, rounds_per_slice pinned at
    16 (the row allows 16 rounds at T <= 3 and 15 at T = 4):
      query 0, T = 1: 17 rounds: slices of 16 and 1
      query 1, T = 3: 41 rounds: slices of 16, 16 and 9.  List 1 lives in slice 0 only, spread evenly (the window
               around the interpolated position holds every cut); list 2 lives in rounds 30 and 31 only: wholly behind
               slice 0, clustered at the end of slice 1 (the window misses, the bisection runs), wholly before slice 2;
               in slices 1 / 2 list 1 and in slices 0 / 2 list 2 have no posting: first and last cut coincide
      query 2, T = 4: 23 rounds: slices of 15 ((15 + 1) * 4 = 64 words: the row exactly) and 8; the first docs of rounds
               3 and 15 (a slice's first boundary) sit in all four lists"""
    one = [ar(0, 17 * 48, 7)]
    three = regular(3, 41, 40, [[10] * 16 + [0] * 25, [0] * 30 + [80, 80] + [0] * 9], 1500)
    four = regular(4, 23, 16, [11, 11, 10], 1500, at_base=(3, 15))
    assert target_for(one, 17) == target_for(three, 41) == target_for(four, 23) == 48
    edges = ["a slice of 1 round", "a slice of 8 rounds", "a slice of 9 rounds", "a slice of 16 rounds",
             "a last slice shorter than the others", "T==1 on the 64-word row", "T==3 on the 64-word row",
             "T==4 on the 64-word row", "(rounds+1)*T==64", "a list with no posting inside a slice",
             "a list wholly before a slice's first boundary", "a list wholly behind a slice's last boundary",
             "a boundary doc that sits in every list", "two-phase: the window holds the cut",
             "two-phase: the window misses and the bisection runs", "two-phase: first and last cut coincide",
             "rows of rounds 8.. replace those of rounds 0..7"]
    return World("cuts4", [segment(62000, one + three + four)], [_ids(0, 1), _ids(1, 3), _ids(4, 4)],
                 dict(uniform_round_target=48, rounds_per_slice=16), edges, 4,
                 n_rounds=[17, 41, 23], n_slices=[2, 3, 2])


@_cached
def cuts8_world():
    """Cut edges on the 128-word row (8-bit instance), rounds_per_slice pinned at 16 (T = 5: 16 rounds fit; T = 8: 15):
      query 0, T = 5: 25 rounds: slices of 16 and 9
      query 1, T = 8: 16 rounds: slices of 15 ((15 + 1) * 8 = 128 words: the row exactly) and 1
      query 2, T = 8: the longest list has 61 postings, the others 59: 474 postings = 10 rounds of stride 7; boundary 9
               lies at position 63 >= 61: it is the end sentinel, round 8 runs to the end and round 9 is empty"""
    five = regular(5, 25, 12, [9, 9, 9, 9], 1000)
    eight = regular(8, 16, 13, [5] * 7, 1000, at_base=(6,))
    tail = [fill(0, 0, 61, gap=10)] + [fill(0, t, 59, gap=10) for t in range(1, 8)]
    assert target_for(five, 25) == target_for(eight, 16) == target_for(tail, 10) == 48
    edges = ["a slice of 1 round", "a slice of 9 rounds", "a slice of 16 rounds", "a last slice shorter than the others",
             "T==5 on the 128-word row", "T==8 on the 128-word row", "(rounds+1)*T==128",
             "a trailing round that is empty", "a boundary doc that sits in every list",
             "two-phase: the window holds the cut", "both header words carry boundaries",
             "rows of rounds 8.. replace those of rounds 0..7"]
    return World("cuts8", [segment(26000, five + eight + tail)], [_ids(0, 5), _ids(5, 8), _ids(13, 8)],
                 dict(uniform_round_target=48, rounds_per_slice=16), edges, 8,
                 n_rounds=[25, 16, 10], n_slices=[2, 2, 1])


# ---- lanes -----------------------------------------------------------------------------------------------------
@_cached
def lanes8_world():
    """Lane edges, T = 8, one slice of 8 rounds of 5 000 docs; list 0 has 64 postings (8 lanes) in every round:
      round 0: lists 1..7 have 0, 1, 7, 8, 9, 0, 5 postings: an empty list between non-empty ones (equal boundary bytes)
      round 1: 64 each: exactly 64 lanes
      round 2: list 1 has 65: exactly 65 lanes, the smallest over-full round
      round 3: 300 each: 2 164 postings = 274 lanes: the header's lane count clamps at 255, first lanes at 127
      rounds 4..7: 3 each; round 5's first doc sits in all eight lists"""
    counts = [[c0, 64, 65 if t == 1 else 64, 300, 3, 3, 3, 3] for t, c0 in zip(range(1, 8), [0, 1, 7, 8, 9, 0, 5])]
    lists = regular(8, 8, 64, counts, 5000, at_base=(5,))
    edges = ["a round of exactly 64 lanes", "a round of exactly 65 lanes", "c==0,1,7,8,9 in one round",
             "an empty list between two non-empty ones", "both header words carry boundaries", "T==8 on the 128-word row",
             "a round of >= 2040 postings: lane count clamps at 255, a first lane at 127", "a slice of 8 rounds",
             "a boundary doc that sits in every list", "need==65", "a chunk that is the rest of the round"]
    return World("lanes8", [segment(40100, lists)], [_ids(0, 8)],
                 dict(uniform_round_target=target_for(lists, 8), rounds_per_slice=8), edges, 8, n_rounds=[8], n_slices=[1])


# ---- chunks ----------------------------------------------------------------------------------------------------
@_cached
def chunks4_world():
    """Chunk edges, T = 3, 6 rounds of 4 000 docs in slices of 3; list 0 has 200 postings (25 lanes) in every round:
      round 0 (a slice's first): all three lists hold the same 200 consecutive docs: 75 lanes; every chunk is cut at a
               doc that all lists hold (the bound doc, in this chunk) and the doc one above it (the next chunk's)
      round 1: 20 + 20
      round 2 (a slice's last): list 1 has 500 consecutive docs, list 2 has 5 early ones: its share of the 61 spare
               lanes rounds to 0, it gets its one lane and finishes in the first chunk while the others do not; the
               later chunks have two lists left
      round 3: 20 + 20
      round 4: 160 + 160: 25 + 20 + 20 = 65 lanes
      round 5: 160 + 152: 64 lanes"""
    span = 4000
    rounds = []
    for r in range(6):
        base = span * r
        rd = {0: fill(base, 0, 200)}
        if r == 0:
            rd = {t: ar(base, 200) for t in range(3)}
        elif r == 2:
            rd[0] = ar(base, 200, 4)
            rd[1] = ar(base + 1, 500)
            rd[2] = base + np.array([3, 9, 15, 21, 27])
        else:
            c = {1: (20, 20), 3: (20, 20), 4: (160, 160), 5: (160, 152)}[r]
            rd[1], rd[2] = fill(base, 1, c[0]), fill(base, 2, c[1])
        rounds.append(rd)
    lists = by_rounds(3, rounds)
    edges = ["need==65", "a round of exactly 65 lanes", "a round of exactly 64 lanes",
             "a chunk in which one list finishes and the others do not", "nne falls between the chunks of a round",
             "a share that rounds to zero extra lanes", "a chunk that is the rest of the round",
             "a doc held by all lists is its chunk's bound doc", "a doc held by all lists one above the bound",
             "an over-full round is a slice's last", "an over-full round is a slice's first",
             "an over-full round at k=257"]
    marks = dict(all_lists=set(range(0, 200)))
    return World("chunks4", [segment(6 * span, lists)], [_ids(0, 3)],
                 dict(uniform_round_target=target_for(lists, 6), rounds_per_slice=3), edges, 4, marks=marks,
                 n_rounds=[6], n_slices=[2])


# ---- filter aliases --------------------------------------------------------------------------------------------
def _alias_world(name, T, ml):
    """4 rounds of 10 000 docs: a round spans more than the filter's period Pd (8 192 docs at 4 list bits, 4 096 at 8).
    Lists A = 0 (16 postings per round), B = 1 (15 in round 0), C = 2 (17 in round 0); round 0:
      d1 in A, d1 + Pd in B: an alias, no partner
      d2 in A and B, d2 + Pd in C: A and B are partners, C's posting is queued beside them and joins nothing
      d3 in A, d3 + 1024 in B: the same word, neighbouring fields: neither is queued
      d4 in A, d4 + k Pd >= 10 000 in B: B's first posting of round 1, which round 0 loads only in the tail of B's last
               lane (15 postings: one spare register): A's posting is queued alone
      d5 and d5 + Pd both in A and nothing else in the field: not queued"""
    Pd = 8192 if ml == 4 else 4096
    d1, d2, d3, d4, d5 = 100, 200, 300, 2004, 500
    tail = d4 + Pd * (-(-(10000 - d4) // Pd))
    assert tail >= 10000 and tail % 16 == 4
    rounds = []
    for r in range(4):
        base = 10000 * r
        rd = {t: fill(base, t, 16 if t < 3 else 8, gap=30) for t in range(T)}
        if r == 0:
            rd[0] = merged(fill(base, 0, 10, gap=30), [d1, d2, d3, d4, d5, d5 + Pd])
            rd[1] = merged(fill(base, 1, 12, gap=30), [d1 + Pd, d2, d3 + 1024])
            rd[2] = merged(fill(base, 2, 16, gap=30), [d2 + Pd])
        if r == 1:
            rd[1] = merged([tail], fill(base, 1, 15, gap=30, skip=2 + (tail - base) // 480))
        if r == 3:
            rd[2] = fill(base, 2, 13, gap=30)      # (list 0 stays the longest)
        rounds.append(rd)
    lists = by_rounds(T, rounds)
    sfx = "" if ml == 4 else " (8 list bits)"
    edges = [e + sfx for e in ["an alias at doc + period is queued without a partner",
                               "partners in A and B with an alias in C: the join sums A and B only",
                               "doc and doc + 1024: neighbouring fields, no interaction",
                               "an alias with a posting behind the round's end in a lane's tail",
                               "two postings of one list that alias each other are not queued"]]
    marks = dict(Pd=Pd, d1=d1, d2=d2, d3=d3, d4=d4, d5=d5, tail=tail)
    return World(name, [segment(40100, lists)], [_ids(0, T)],
                 dict(uniform_round_target=target_for(lists, 4), rounds_per_slice=2, champions=0), edges, ml, marks=marks,
                 n_rounds=[4], n_slices=[2])


@_cached
def alias4_world():
    """_alias_world on the 4-bit instance (T = 3, period 8 192)"""
    return _alias_world("alias4", 3, 4)


@_cached
def alias8_world():
    """_alias_world on the 8-bit instance (T = 5, period 4 096)"""
    return _alias_world("alias8", 5, 8)


# ---- join ------------------------------------------------------------------------------------------------------
JOIN4_QUEUES = (0, 8, 56, 57, 63, 64, 65, 128, 129, 130, 1)


@_cached
def join4_world():
    """Join edges, T = 3, no champion seed and one round per slice (fewer than 256 docs: at k >= 256 no threshold ever
    forms and every round queues exactly its shared docs).  List 0 has 72 postings per round; round r queues
    JOIN4_QUEUES[r] entries, made of docs shared by lists 0 and 1, by lists 0 and 2 (first and last list only) and by
    all three:
      0, 8, 56, 57, 63, 64: the all-pairs join, with its padded last group (57, 63) and a full wave (64)
      65, 128, 129, 130: the binary-search join with 2, 2, 3 and 3 receiver blocks of 64 (one block is the all-pairs
               join's: the search join starts at 65 entries); at 128 and 130 list 1 has no queued
               entry between two lists that have 64 and 65 (the longest segment: the step count)
      1: the last round; list 0 holds a doc = 8191 mod 8192, the field of the sentinels that pad list 2's last lane"""
    recipe = {0: (0, 0, 0), 8: (4, 0, 0), 56: (28, 0, 0), 57: (27, 0, 1), 63: (0, 30, 1), 64: (32, 0, 0),
              65: (0, 31, 1), 128: (0, 64, 0), 129: (63, 0, 1), 130: (0, 65, 0), 1: (0, 0, 0)}
    rounds = []
    for r, n in enumerate(JOIN4_QUEUES):
        base = 2000 * r if n != 1 else 24000
        p01, p02, tr = recipe[n]
        a = fill(base, 0, 72)
        rd = {0: a, 1: merged(a[:p01], a[70:70 + tr], fill(base, 1, 4 if n != 1 else 8)),
              2: merged(a[:p02], a[70:70 + tr], fill(base, 2, 4))}
        if n == 1:
            rd[0] = merged(a[:71], [3 * 8192 - 1])
        rounds.append(rd)
    lists = by_rounds(3, rounds)
    edges = [f"a queue of {n} entries" for n in JOIN4_QUEUES] + \
        ["two receiver blocks", "three receiver blocks", "a doc in all T lists",
         "a doc in the first and last list only", "dense join: a list with no queued entry between two that have some",
         "a longest queue segment of 64", "a longest queue segment of 65", "an alias with the sentinels behind a list"]
    nr = len(JOIN4_QUEUES)
    return World("join4", [segment(26000, lists)], [_ids(0, 3)],
                 dict(uniform_round_target=target_for(lists, nr), rounds_per_slice=1, champions=0), edges, 4,
                 n_rounds=[nr], n_slices=[nr])


@_cached
def pad4_world():
    """The padded last group of the all-pairs join, T = 3, no seed, one round per slice.  Round 0 queues 57 entries, so
    the join reads entries 57..63 as well: LDS words 114..127, which hold FILTER words unless the kernel overwrites them
    with entries no doc matches.  Doc 114 of list 0 leaves the word 1 at entry 57's doc, doc 115 + 7 * 1024 of list 2
    leaves the bits of 2.0f at its score, and doc 1 is queued (lists 0 and 1): without the padding doc 1 gains 2.0."""
    a = fill(0, 0, 72)
    r0 = {0: merged(a[:70], [1, 114]), 1: merged([1], a[1:27], a[60:61], fill(0, 1, 4)),
          2: merged(a[60:61], fill(0, 2, 4), [115 + 7 * 1024])}
    r1 = {0: fill(8000, 0, 72), 1: fill(8000, 1, 4), 2: fill(8000, 2, 4)}
    lists = by_rounds(3, [r0, r1])
    edges = ["a queue of 57 entries", "a filter word behind the queue equals a queued doc"]
    return World("pad4", [segment(10000, lists)], [_ids(0, 3)],
                 dict(uniform_round_target=target_for(lists, 2), rounds_per_slice=1, champions=0), edges, 4,
                 n_rounds=[2], n_slices=[2])


def _join8_lists():
    """T = 8, 5 rounds of 2 000 docs, list 0 has 32 postings per round:
      round 0: 9 docs in all eight lists: 72 entries, the binary-search join over both halves of the lists
      round 1: 8 docs in all eight lists: 64 entries, the all-pairs join's full wave
      round 2: 2 docs in the first and last list only; lists 2 and 3 have no posting (a leaf without a lane)
      round 3: 2 docs in lists 0 and 1 only, 2 docs in lists 0, 1 and 2: 10 entries
      round 4: 14 docs in lists 0 and 1 only, 14 in lists 0, 1 and 2: 70 entries"""
    rounds = []
    for r in range(5):
        base = 2000 * r
        a = fill(base, 0, 32)
        rd = {0: a}
        for t in range(1, 8):
            own = fill(base, t, 2)
            if r < 2:
                rd[t] = merged(a[1:10 - r], own)
            elif r == 2:
                rd[t] = merged(a[1:3], own) if t == 7 else ([] if t in (2, 3) else own)
            else:
                n = 2 if r == 3 else 14
                rd[t] = merged(a[1:1 + 2 * n], own) if t == 1 else merged(a[1 + n:1 + 2 * n], own) if t == 2 else own
        rounds.append(rd)
    return by_rounds(8, rounds)


@_cached
def join8_world():
    """_join8_lists as a flat sum, no seed, one round per slice: T = 8, so both halves of the four-at-a-time search
    run."""
    lists = _join8_lists()
    edges = ["a queue of 72 entries over 8 lists", "a queue of 64 entries", "a doc in all T lists",
             "a doc in the first and last list only", "two receiver blocks", "both header words carry boundaries"]
    return World("join8", [segment(10100, lists)], [_ids(0, 8)],
                 dict(uniform_round_target=target_for(lists, 5), rounds_per_slice=1, champions=0), edges, 8,
                 n_rounds=[5], n_slices=[5])


# ---- plans -----------------------------------------------------------------------------------------------------
PLANS8 = [  # (leaf of every list, plan, tie, leaves, min_match, weight of list 7)
    ([0, 0, 1, 1, 2, 2, 3, 3], PLAN_SUM, 0.0, 4, 0, 2.25),
    ([0, 0, 1, 1, 2, 2, 3, 3], PLAN_DISMAX, 0.3, 4, 0, 2.25),
    ([0] * 8, PLAN_SUM, 0.0, 1, 0, 2.25),
    (list(range(8)), PLAN_DISMAX, 0.5, 8, 0, 2.25),
    ([0, 0, 0, 0, 1, 1, 1, 1], PLAN_DISMAX, 0.25, 2, 0, 2.25),
    ([0, 0, 1, 1, 2, 2, 3, 3], PLAN_SUM, 0.0, 4, 2, 2.25),
    ([0, 0, 1, 1, 2, 2, 3, 3], PLAN_SUM, 0.0, 4, 0, -0.5),
]


@_cached
def plans8_world():
    """The PLAN instantiation over join8's queues (both join forms), and a second, small segment that lacks term 3.
    The queries of PLANS8: a flat Sum and a flat DisMax of four two-list leaves; all lists in one leaf; every list its
    own leaf (in segment 1 leaf 3 has no term: max_init); a leaf boundary between lists 4 and 5 (the two header words);
    min_match 2 over the docs of rounds 3 and 4 (lists 0 and 1 only: two lists, ONE leaf: rejected; lists 0, 1 and 2:
    two leaves: accepted); a negative weight on list 7.  In round 2 leaf 1 (lists 2, 3) has no lane."""
    lists = _join8_lists()
    small = [ar(3 + (t % 3), 12 + t, 7) for t in range(7)]
    segs = [segment(10100, lists), segment(200, small, seed=2)]
    queries, leaf = [], []
    for lf, _, _, _, _, w7 in PLANS8:
        queries.append([([t, NO_TERM if t == 3 else t - (t > 3)], w7 if t == 7 else 0.5 + 0.25 * t) for t in range(8)])
        leaf += lf
    plans = dict(q_leaf=np.array(leaf, np.uint32), q_plan=np.array([p[1] for p in PLANS8], np.int32),
                 q_tie=np.array([p[2] for p in PLANS8], np.float32), q_nleaves=np.array([p[3] for p in PLANS8], np.uint32),
                 q_min_match=np.array([p[4] for p in PLANS8], np.uint32))
    edges = ["plan: a flat Sum, both join forms", "plan: a flat DisMax with a tie breaker, both join forms",
             "plan: all lists in one leaf", "plan: every list its own leaf", "plan: a leaf boundary between lists 4 and 5",
             "plan: a leaf none of whose lists has a lane in the round",
             "plan: min_match 2, a doc in two lists of one leaf only", "plan: min_match 2, the same with a second leaf",
             "plan: a negative weight", "plan: a leaf whose term is absent from one of two segments"]
    return World("plans8", segs, queries, dict(uniform_round_target=target_for(lists, 5), rounds_per_slice=1, champions=0),
                 edges, 8, plans=plans)


# ---- threshold -------------------------------------------------------------------------------------------------
def _flat_lengths(seg):
    """every doc the same length: a posting's impact depends on its tf (doc mod 5 + 1) and its list alone, so scores
    repeat bit for bit"""
    seg.field_doc_len = [np.full(seg.n_docs, 20.0, dtype=np.float32)]
    seg.field_avgdl = np.array([20.0], dtype=np.float32)
    return seg


THRESHOLD_KS = (3, 30, 90)


def _threshold_world(name, champions, filtered):
    """T = 3 over docs of one length: list 0 every 2nd doc, list 1 every 5th, list 2 every 7th of 1 400 (list 0 has the 512
    postings a seed at k = 257 needs).  Scores take
    few distinct values, so at the k of THRESHOLD_KS docs with identical score bits lie on both sides of rank k (the
    lower doc wins), among them singles whose weight * impact has the threshold's bits and joined docs whose sum has."""
    lists = [ar(0, 700, 2), ar(0, 280, 5), ar(1, 200, 7)]
    seg = _flat_lengths(segment(1500, lists))
    edges = {(1, False): ["threshold: identical score bits on both sides of rank k", "threshold: the champion seed on",
                          "threshold: k=257 with a seed", "threshold: a single tied with the doc at rank k",
                          "threshold: a joined doc tied with the doc at rank k"],
             (0, False): ["threshold: the champion seed off", "threshold: k=257 without a seed"],
             (1, True): ["threshold: a doc filter keeps the seed off"]}[(champions, filtered)]
    masks = None
    if filtered:
        masks = [np.arange(1500) % 4 != 1]
    return World(name, [seg], [_ids(0, 3)], dict(champions=champions, rounds_per_slice=4), edges, 4,
                 strategies=(BM25, WAND), ks=THRESHOLD_KS, masks=masks)


@_cached
def threshold_world():
    """_threshold_world with the champion seed"""
    return _threshold_world("threshold", 1, False)


@_cached
def threshold_noseed_world():
    """_threshold_world without champions: the threshold grows from the top-k buffer alone"""
    return _threshold_world("threshold_noseed", 0, False)


@_cached
def threshold_filter_world():
    """_threshold_world with a doc filter on the query: the planner gives no seed"""
    return _threshold_world("threshold_filter", 1, True)


@_cached
def tiejoin4_world():
    """The join's threshold test on a LIVE threshold with the candidate's own bits, T = 2, no seed, docs of one length.
    Round 0 spans docs [0, 9 000): list 0 (weight 2) holds doc 4 and 207 docs 9 + 40 i, all with tf 5: 208 equal scores.
    List 1 (weight 0.01) holds 8 196 = 4 + 8 192: doc 4 is queued as an alias, the other 207 are singles.  They are
    taken before the join, 26 or 27 per register, and overflow the top-k buffer (128 entries at k <= 64, 192 at
    k = 65): it compacts and the threshold becomes (that score, the lowest single's doc).  Doc 4 then reaches the
    join's candidate site with exactly the threshold's score and a lower doc id: it must be taken, and is rank 1."""
    r0 = {0: merged([4], 9 + 40 * np.arange(207)), 1: merged([4 + 8192], 8192 + 10 + 40 * np.arange(5))}
    r1 = {0: 9000 + 40 * np.arange(208), 1: 9010 + 40 * np.arange(6)}
    lists = by_rounds(2, [r0, r1])
    edges = ["threshold: a joined entry meets a compacted threshold of its own score bits with a lower doc id"]
    return World("tiejoin4", [_flat_lengths(segment(18000, lists))], [[(0, 2.0), (1, 0.01)]],
                 dict(uniform_round_target=target_for(lists, 2), rounds_per_slice=2, champions=0), edges, 4,
                 strategies=(BM25, WAND), n_rounds=[2], n_slices=[1])


def _adjacent_weights(imp0, imp1):
    """weights (w0, w1) with f32(w1 * imp1) exactly one ulp below f32(w0 * imp0)"""
    F32 = np.float32
    for j in range(4096):
        w0 = F32(1.0) + F32(j) * F32(2.0 ** -12)
        want = np.nextafter(F32(w0 * imp0), F32(0))
        w1 = F32(want / imp1)
        for _ in range(4):
            w1 = np.nextafter(w1, F32(0))
        for _ in range(9):
            if F32(w1 * imp1) == want:
                return float(w0), float(w1)
            w1 = np.nextafter(w1, F32(4))
    raise AssertionError("no adjacent pair of weighted impacts")


@_cached
def ulp4_world():
    """A single with exactly the threshold's bits and one a bit below, T = 2 over docs of one length, champion seed on,
    k = 1.  The lists share no doc; every posting has tf 5, so a list's postings all carry its maximum impact.  The
    weights are searched so that w1 * impact1 is the float just below w0 * impact0 = the seed theta0.  List 1 (the
    lower score) has the lower doc ids: rank 1 is list 0's first doc, whatever order the candidates arrive in."""
    from tests import stage_ref
    lists = [1009 + 10 * np.arange(120), 4 + 10 * np.arange(100)]
    seg = _flat_lengths(segment(2300, lists))
    imp = stage_ref.impacts_np(seg)
    assert len(set(imp[:120].tolist())) == 1 and len(set(imp[120:].tolist())) == 1
    w0, w1 = _adjacent_weights(imp[0], imp[120])
    edges = ["threshold: a single with the seed's bits and a single one ulp below"]
    return World("ulp4", [seg], [[(0, w0), (1, w1)]], dict(champions=1, rounds_per_slice=4), edges, 4,
                 strategies=(BM25, WAND))


@_cached
def guess4_world():
    """The global guess's own miss path, T = 2, 7 rounds of 10 000 docs in slices of 4 and 3 (no interpolation: every
    cut is lower_bound_guess's).  List 1 has 600 postings, all in round 5: at every boundary the position a uniform
    spread predicts is hundreds of postings off, the 128-posting window misses, the bracket widens (600 > 512) and
    bisects."""
    lists = regular(2, 7, 100, [[0, 0, 0, 0, 0, 600, 0]], 10000)
    edges = ["the global guess misses: its bracket widens and bisects"]
    return World("guess4", [segment(70000, lists)], [_ids(0, 2)],
                 dict(uniform_round_target=target_for(lists, 7), rounds_per_slice=4), edges, 4, n_rounds=[7], n_slices=[2])


WORLDS = (cuts4_world, cuts8_world, lanes8_world, chunks4_world, alias4_world, alias8_world, join4_world, pad4_world, join8_world,
          plans8_world, threshold_world, threshold_noseed_world, threshold_filter_world, tiejoin4_world, ulp4_world,
          guess4_world)
