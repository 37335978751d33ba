"""The world of tests/test_gpu_collapse.py, built without a device so that tests/test_collapse_world.py can check on
the CPU, with tests/collapse_ref.py alone, that it gives what the GPU cases need.

Segments of 300 / 200 / 120 docs over a vocabulary of 40 (the second with tombstones), 16 three-term queries — query
0 asks for the three most frequent terms and matches nearly every live doc, query 14 has no term, query 15 matches a
single doc — two sort fields and six keyword columns."""
import copy
import math
import struct

import numpy as np

from tests import collapse_ref as R
from tests.util import _append_lists, random_queries, random_segment

NO_TERM = 0xFFFFFFFF
KS = (1, 2, 63, 64, 65, 255, 256, 257, 620)
# None: no inner hits; else (from, size).  (600, 1) is beyond SLG_MAX_INNER_HITS: the library must refuse it;
# (63, 1) is the largest `from` it takes, at or beyond the members of most groups
INNERS = (None, (0, 1), (0, 64), (1, 63), (3, 2), (600, 1), (63, 1))
MAX_INNER_HITS = 64
NAN = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]
BIG_ORDS = 1 << 20


def tombstoned(seg, rng, frac):
    s = copy.copy(seg)
    dead = rng.random(seg.n_docs) < frac
    s.deleted = np.packbits(dead, bitorder="little")
    s.docs = float(seg.n_docs - int(dead.sum()))
    return s


def make_fields(rng, n_docs):
    """`low`: an i64 of 8 values on every doc, so its ties are long and fall to (segment, doc); `f64`: 0 .. 2 values
    per doc out of a pool with NaN, -0.0 and infinities (a doc without one is Missing)"""
    pool = [0.0, -0.0, 1.5, -1.5, 3.0, math.inf, -math.inf, NAN]
    low = [[[int(rng.integers(0, 8))] for _ in range(n)] for n in n_docs]
    f64 = [[[pool[j] for j in rng.integers(0, len(pool), int(rng.integers(0, 3)))] for _ in range(n)] for n in n_docs]
    return {"low": (low, False), "f64": (f64, True)}


def make_columns(rng, n_docs):
    """name -> (per segment: one list of ordinals per doc, or None = the segment has no column; n_ords)"""
    total = sum(n_docs)
    base = np.concatenate([[0], np.cumsum(n_docs)])
    seven = [[[] if rng.random() < 0.1 else [int(rng.integers(0, 7))] for _ in range(n)] for n in n_docs]
    multi = [[list(v) for v in col] for col in seven]
    for s, n in enumerate(n_docs):  # a few docs with two values
        for d in rng.choice(n, size=max(2, n // 60), replace=False):
            multi[s][int(d)] = [int(rng.integers(0, 7)), int(rng.integers(0, 7))]
    # multiples of 8192 and of 8192 + 1: equal low bits, so probe chains form at every table size
    big = [[[int(rng.integers(0, 96)) * 8192 + int(rng.integers(0, 2))] for _ in range(n)] for n in n_docs]
    return {
        "seven": (seven, 7),
        "one": ([[[0]] * n for n in n_docs], 1),
        "own": ([[[int(base[s]) + d] for d in range(n)] for s, n in enumerate(n_docs)], total),
        "big": (big, BIG_ORDS),
        "noseg": ([None if s == 1 else col for s, col in enumerate(seven)], 7),
        "multi": (multi, 7),
    }


def sorted_rows(all_hits, sort, fields):
    """the oracle's hits with k >= the docs -> per query [(seg, doc, score)] in the order of `sort` (None: score
    order, as they are); a sort without a `_score` part leaves the scores 0.0 (ScoreMode::MatchOnly)"""
    doc, seg, score, count = all_hits
    out = []
    for q in range(len(count)):
        hits = [(int(seg[q, i]), int(doc[q, i]), score[q, i]) for i in range(int(count[q]))]
        if sort is not None:
            hits.sort(key=R.sort_key(sort, fields))
            if not any(p == "_score" for p, _ in sort):
                hits = [(s, d, np.float32(0.0)) for s, d, _ in hits]
        out.append(hits)
    return out


def as_arrays(rows, k):
    """per query rows cut at k -> (doc, seg, score [nq, k], count [nq]) as slg_batch_fetch returns them"""
    nq = len(rows)
    doc, seg = np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.uint32)
    score, count = np.zeros((nq, k), np.float32), np.zeros(nq, np.uint32)
    for q, hits in enumerate(rows):
        hits = hits[:k]
        count[q] = len(hits)
        for i, (s, d, sc) in enumerate(hits):
            seg[q, i], doc[q, i], score[q, i] = s, d, sc
    return doc, seg, score, count


def build(oracle, big=False):
    """big: a fourth segment of 5000 docs, so that query 0 has more than 4096 rows"""
    rng = np.random.default_rng(20261)
    sizes = (300, 200, 120) + ((5000,) if big else ())
    segs = [random_segment(rng, n, 40, 25, k1=0.9, b=0.4) for n in sizes]
    segs[0] = _append_lists(segs[0], [([17], [2])])  # term 40 of segment 0 is in one doc
    segs[1] = tombstoned(segs[1], rng, 0.15)
    n_segs = len(segs)
    offs, terms, w = random_queries(rng, 16, 3, 40, n_segs=n_segs, weights=True)
    terms[0:3, :] = np.array([0, 1, 2], np.uint32)[:, None]  # query 0: the most frequent terms
    terms[14 * 3:15 * 3, :] = NO_TERM                        # query 14: no term
    terms[15 * 3:16 * 3, :] = NO_TERM                        # query 15: one doc
    terms[15 * 3, 0] = 40
    n_docs = [s.n_docs for s in segs]
    k_all = sum(n_docs)
    all_hits = oracle.search_batch(segs, offs, terms, w, k_all, strategy=oracle.BM25)
    return dict(segs=segs, offs=offs, terms=terms, w=w, n_docs=n_docs, k_all=k_all, all=all_hits,
                fields=make_fields(rng, n_docs), columns=make_columns(rng, n_docs))
