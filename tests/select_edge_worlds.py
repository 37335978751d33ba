"""The worlds of the select kernels' edge tests: plain data, no device (test infrastructure).

tests/test_gpu_select_edges.py runs them on the device; tests/test_select_edges_worlds.py proves on the CPU that they
have the properties the device cases rest on (candidate counts, tie structure, slice counts, region pattern).

Every query is a single crafted list per segment (tests.util._append_lists), so its candidate count n is the
list's length, exactly.  The constants below restate searchlite_amd/csrc/slg_kernels.hpp.
"""
import copy

import numpy as np

from tests.util import TOPK_ROUND_PER_SLICE, _append_lists

NO_TERM = 0xFFFFFFFF
SELECT_CAP = 2048      # kSelectCap: keys of one rank range of select_topk_kernel
SORTED_CAP = 1024      # kSortedCap: the same of select_sorted_kernel
MAX_SLICES = 512       # kSelectMaxSlices: slice table in LDS up to here, the strided loop beyond
SELECT_THREADS = 512   # kSelectThreads: n_flat > 16 * NT forces cap_last = kSelectCap

# no threshold seed and one round per slice: every posting of a list is a candidate (tests.util.topk_variants "b")
NO_SEED = dict(TOPK_ROUND_PER_SLICE)
SLICE_TUNING = dict(NO_SEED, uniform_round_target=48)     # one slice per round of 48 postings
REGION_TUNING = dict(NO_SEED, uniform_round_target=128)   # regions of 128: room for 64 survivors and for 128

TOPK_KS = (2047, 2048, 2049, 4096, 4097, 6145)
SORTED_KS = (1023, 1024, 1025, 2048, 2049, 3073)
SMALL_KS = (1, 63, 64, 65, 128, 129)
N_BIG = 9000           # well above every k
TOPK_NS = sorted({k + d for k in TOPK_KS for d in (-1, 0, 1)}) + [N_BIG]
SORTED_NS = sorted({k + d for k in SORTED_KS for d in (-1, 0, 1)}) + [N_BIG]
SWITCH_NS = (16 * SELECT_THREADS, 16 * SELECT_THREADS + 1)   # the two sides of n_flat > 16 * NT
SWITCH_KS = (257, 2049)
SLICE_COUNTS = (1, 2, 2, 511, 512, 513, 700)                 # of SLICE_QUERIES, over all segments
SLICE_QUERIES = ("s1", "s2", "s2one", "s511", "s512", "s513", "s700")
SLICE_KS = (257, 2049)
# survivors of the MUST list per region of list "E": empty at the start, in the middle (two in a row), at the end
REGION_SURVIVORS = ([0, 1, 64, 0, 0, 128, 1, 0, 64, 0], [0, 5, 0])
REGION = 128


def last_range_cap(left, cap):
    """last_range_cap of slg_kernels.hpp: powers of two from 64, at most cap"""
    c = 64
    while c < left:
        c <<= 1
    return min(c, cap)


def overshoot_ns(k):
    """n on both sides of the `all` shortcut at k, and one that leaves a select with an overshoot"""
    cap_last = last_range_cap(k, SELECT_CAP)
    return (cap_last, cap_last + 1, 2 * cap_last + 1)


OVERSHOOT_NS = sorted({n for k in SMALL_KS for n in overshoot_ns(k)})


def _segment(rng, n_docs, const_dl=None):
    """a segment whose vocabulary is one term (doc 0); const_dl: every doc as long as the average"""
    from searchlite_amd.segment import Segment
    dl = np.full(n_docs, const_dl, np.float32) if const_dl else rng.integers(3, 10, size=n_docs).astype(np.float32)
    avg = np.float32(np.float32(dl.sum()) / np.float32(n_docs))
    return Segment(n_docs=n_docs, term_offsets=np.array([0, 1], np.uint64), doc_ids=np.array([0], np.uint32),
                   tfs=np.array([1], np.uint32), field_doc_len=[dl], field_avgdl=np.array([avg], np.float32),
                   docs=float(n_docs), k1=1.2, b=0.75)


def _pick(rng, lo, hi, n):
    return np.sort(rng.choice(np.arange(lo, hi), size=n, replace=False)).astype(np.uint32)


class World:
    """segs; T[name] = the list's term id per segment (NO_TERM where it has none); n[name] = its postings"""

    def __init__(self, rng, segs, lists, const_tf):
        per_seg = [[] for _ in segs]
        self.T, self.n, self.lists = {}, {}, lists
        for name, parts in lists.items():
            ids = []
            for s, d in enumerate(parts):
                if d is None:
                    ids.append(NO_TERM)
                    continue
                ids.append(segs[s].n_terms + len(per_seg[s]))
                per_seg[s].append((d, np.ones(len(d), np.uint32) if const_tf else rng.integers(1, 4, size=len(d))))
            self.T[name] = ids
            self.n[name] = sum(len(d) for d in parts if d is not None)
        self.segs = [_append_lists(sg, per_seg[s]) for s, sg in enumerate(segs)]
        self.k_all = sum(sg.n_docs for sg in segs)
        self.fields = {}

    def queries(self, names):
        """one single-term query per name -> (q_offsets, q_terms [nq, n_segs], q_weights)"""
        return (np.arange(len(names) + 1, dtype=np.uint32), np.array([self.T[nm] for nm in names], np.uint32),
                np.ones(len(names), np.float32))

    def tombstoned(self, seg, seed):
        """a copy with every ~10th doc of `seg` deleted (live_docs kept, so the scores stay)"""
        w = copy.copy(self)
        w.segs = list(self.segs)
        w.segs[seg] = copy.copy(self.segs[seg])
        dead = np.random.default_rng(seed).random(w.segs[seg].n_docs) < 0.1
        w.segs[seg].deleted = np.packbits(dead, bitorder="little")
        return w

    def masks(self, seed):
        rng = np.random.default_rng(seed)
        return [rng.random(sg.n_docs) < 0.6 for sg in self.segs]


def third_filtered(nq, fid):
    """a doc filter on a third of the queries"""
    return np.array([fid if q % 3 == 1 else -1 for q in range(nq)], np.int32)


_worlds = {}


def _cached(fn):
    def get():
        if fn.__name__ not in _worlds:
            _worlds[fn.__name__] = fn()
        return _worlds[fn.__name__]
    return get


@_cached
def ranges_world():
    """Cases 1, 2 and 6.  Two segments of 10 000 and 8 000 docs with random lengths and tfs (a handful of distinct
    scores: ties everywhere).  For every n of TOPK_NS and SORTED_NS list "a<n>" has its n docs in segment 0 and list
    "b<n>" a third of them in segment 0, the rest in segment 1.  Sort fields as tests/test_gpu_sort.make_fields."""
    from tests.test_gpu_sort import make_fields
    rng = np.random.default_rng(8101)
    segs = [_segment(rng, 10_000), _segment(rng, 8_000)]
    lists = {}
    for n in sorted(set(TOPK_NS) | set(SORTED_NS)):
        lists[f"a{n}"] = [_pick(rng, 0, 10_000, n), None]
        lists[f"b{n}"] = [_pick(rng, 0, 10_000, n // 3), _pick(rng, 0, 8_000, n - n // 3)]
    W = World(rng, segs, lists, const_tf=False)
    W.fields = make_fields(rng, W.segs)
    W.topk_names = [f"{v}{n}" for n in TOPK_NS for v in "ab"]
    W.sorted_names = [f"{v}{n}" for n in SORTED_NS for v in "ab"]
    return W


@_cached
def ties_world():
    """Cases 3 and 4.  Three segments of 1 800, 9 000 and 4 000 docs, every doc as long as the average and every tf
    1: the postings of a list have one impact per segment, and a list that holds more than half of a segment's docs
    has idf 1 there (the logarithm is clamped at 0), so "tie_topk" (1 000 + 5 145 docs of segments 0 and 1) and
    "tie_x" / "tie_y" (1 000 + 2 073 docs of segments 0 and 2) score one bit pattern over both their segments.
    Columns: "const" (7 everywhere) and "two" (0 below doc 900 / any / 2 000 of segment 0 / 1 / 2, else 1): tie_x
    holds 1 024 docs with a 0, tie_y 1 025.  Lists "o<n>" (segment 1 alone): the counts around the `all`
    shortcut, and 8 192 / 8 193 for the large-candidate switch."""
    rng = np.random.default_rng(8102)
    segs = [_segment(rng, 1_800, 4.0), _segment(rng, 9_000, 4.0), _segment(rng, 4_000, 4.0)]

    def xy(zeros0):
        return [np.concatenate([_pick(rng, 0, 900, zeros0), _pick(rng, 900, 1_800, 1_000 - zeros0)]), None,
                np.concatenate([_pick(rng, 0, 2_000, 512), _pick(rng, 2_000, 4_000, 1_561)])]

    lists = {"tie_topk": [_pick(rng, 0, 1_800, 1_000), _pick(rng, 0, 9_000, 3 * SELECT_CAP + 1 - 1_000), None],
             "tie_x": xy(512), "tie_y": xy(513)}
    for n in list(OVERSHOOT_NS) + list(SWITCH_NS):
        lists[f"o{n}"] = [None, _pick(rng, 0, 9_000, n), None]
    W = World(rng, segs, lists, const_tf=True)
    W.fields = {"const": ([[[7]] * sg.n_docs for sg in W.segs], False),
                "two": ([[[0 if d < lim else 1] for d in range(sg.n_docs)]
                         for sg, lim in zip(W.segs, (900, 9_000, 2_000))], False)}
    return W


@_cached
def slices_world():
    """Cases 5 and 6.  Two segments of 18 000 docs.  Under SLICE_TUNING a list of 48 * s postings is s slices:
    SLICE_QUERIES have SLICE_COUNTS slices over both segments.  Under REGION_TUNING list "E" (docs 0 .. 1 279 of
    segment 0, 0 .. 383 of segment 1) is 10 + 3 regions of 128 consecutive docs, of which the MUST list "M" keeps
    REGION_SURVIVORS.  Column "low": doc % 8."""
    rng = np.random.default_rng(8103)
    N = 18_000
    segs = [_segment(rng, N), _segment(rng, N)]
    two = lambda a, b: [_pick(rng, 0, N, 48 * a), _pick(rng, 0, N, 48 * b)]
    lists = {"s1": [_pick(rng, 0, N, 30), None], "s2": [_pick(rng, 0, N, 30), _pick(rng, 0, N, 30)],
             "s2one": [_pick(rng, 0, N, 96), None], "s511": two(256, 255), "s512": two(256, 256),
             "s513": two(257, 256), "s700": two(350, 350)}
    lists["E"] = [np.arange(REGION * len(r), dtype=np.uint32) for r in REGION_SURVIVORS]
    lists["M"] = [np.concatenate([np.arange(REGION * j + (REGION - c) // 2, REGION * j + (REGION - c) // 2 + c)
                                  for j, c in enumerate(r)]).astype(np.uint32) for r in REGION_SURVIVORS]
    W = World(rng, segs, lists, const_tf=False)
    W.fields = {"low": ([[[d % 8] for d in range(N)] for _ in W.segs], False)}
    return W


def region_clauses(W):
    """the bool batch of the empty-region case: query 0 = list E under MUST M, query 1 = E with no clause"""
    from tests import bool_ref as B
    return B.clauses_of([([(B.MUST, [tuple(W.T["M"])])], 0), ([], 0)], len(W.segs))


def accepting_clauses(nq, n_segs):
    """clause tables that accept every doc: none at all (even queries), a MUST_NOT group of an absent term (odd)"""
    from tests import bool_ref as B
    return B.clauses_of([([], 0) if q % 2 == 0 else ([(B.MUST_NOT, [(NO_TERM,) * n_segs])], 0) for q in range(nq)],
                        n_segs)
