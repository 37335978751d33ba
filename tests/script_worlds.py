"""The worlds of tests/test_gpu_script.py: segments, an index over them, registered columns and filters by name, the
reference's view of both (tests/fscore_ref.Columns) and the expected result of a script batch (tests/script_ref.apply
over the oracle's exhaustive run, which is made once per query set and shared).

world_a(): the two small tombstoned segments of the function_score tests — 300 and 200 docs, vocab 40.  Columns:
  pop   f64, 0-3 values per doc (the first counts; some docs have none)
  age   i64, one value per doc in 0..5000 (stored without offsets; some are 0)
  half  f64 whose second segment has no offsets at all (every doc of it is without a value)
  zed   f64 over 0.0, -0.0, 1.0, -2.0, 0.5 (divisors)
  c0 .. c4  i64 in -3..3 (more distinct fields)
world_b(): one segment of 6000 docs with appended lists of 1, 63, 64, 65, 129 and 6000 docs (one slice each but the
last).  Columns: rank i64 (a doc of the 129-list: its rank in the list; else 1000), parity f64 (doc & 1), and keepM
f64 for M in 0, 1, 63, 64, 65: 1.0 for the docs of the 129-list with rank >= 129 - M and for every doc outside the
list, else 0.0 — `_score / keepM` leaves M of the 129."""
import numpy as np

from searchlite_amd.script import compile_script
from tests import fscore_ref, script_ref
from tests.test_gpu_bool import csr, dead_bitmap, same
from tests.util import _append_lists, random_queries, random_segment

F32 = np.float32
KEEPS = (0, 1, 63, 64, 65)


class World:
    def __init__(self, sa, oracle, segs, **tuning):
        self.oracle, self.segs, self.n_segs = oracle, segs, len(segs)
        self.ix = sa.GpuIndex(segs, **tuning)
        self.cols = fscore_ref.Columns(segs)
        self.F, self.flt, self._cands = {}, {}, {}

    def add_field(self, name, per_seg, dtype):
        fid = self.ix.add_agg_field(per_seg, dtype)
        self.F[name] = fid
        self.cols.fields[fid] = (per_seg, np.dtype(dtype))
        return fid

    def add_filter(self, name, masks):
        fid = self.ix.add_filter(masks)
        self.flt[name] = fid
        self.cols.filters[fid] = masks
        return fid

    def script(self, text, boost=1.0, **params):
        """a script over the world's columns by name -> the entry of script_spec()"""
        return dict(program=compile_script(text, params or None, self.F), boost=boost)

    def cands(self, qs, plans):
        key = (id(qs), tuple(sorted(plans)))
        if key not in self._cands:  # (one exhaustive oracle run per query set, shared by the checks)
            self._cands[key] = (qs, fscore_ref.all_candidates(self.oracle, self.segs, *qs, **plans))
        return self._cands[key][1]

    @staticmethod
    def chains(scripts, fscore=None, order="outer"):
        """per query the stages in the order they run"""
        out = []
        for q, sc in enumerate(scripts):
            stages = [("script", sc)]
            if fscore is not None:
                fs = ("fscore", fscore[q])
                stages = [fs] + stages if order == "outer" else stages + [fs]
            out.append(stages)
        return out

    def want(self, qs, scripts, k, fscore=None, order="outer", q_filter=None, **plans):
        """-> ((doc, seg, score, count), scored_docs, matched, ranked survivors)"""
        return script_ref.apply(self.cands(qs, plans), self.segs, self.chains(scripts, fscore, order), self.cols, k, q_filter)

    def check(self, qs, scripts, k, what, fscore=None, order="outer", q_filter=None, **plans):
        """a script batch in score order, with stats -> (got, scored_docs, matched)"""
        want, scored, matched, _ = self.want(qs, scripts, k, fscore, order, q_filter, **plans)
        got = self.ix.search_batch_script(*qs, k, scripts, fscore=fscore, script_order=order, want_stats=True,
                                          q_filter=q_filter, **plans)
        same(got[:4], want, what)
        got_sd = [int(got[4][q].scored_docs) for q in range(len(scored))]
        assert got_sd == scored.tolist(), f"{what}: scored_docs {got_sd} != {scored.tolist()}"
        assert [int(got[4][q].candidates_examined) for q in range(len(scored))] == scored.tolist()
        return got, scored, matched


def world_a(sa, oracle):
    rng = np.random.default_rng(17)
    segs = [random_segment(rng, 300, 40, 6), random_segment(rng, 200, 40, 6)]
    segs[0].deleted = dead_bitmap(rng, 300, 0.1)
    segs[1].deleted = dead_bitmap(rng, 200, 0.15)
    W = World(sa, oracle, segs)
    W.add_field("pop", [[[float(rng.uniform(0.1, 1000.0)) for _ in range(int(rng.integers(0, 4)))] for _ in range(s.n_docs)]
                        for s in segs], np.float64)
    W.add_field("age", [[[int(rng.integers(0, 5001)) if rng.random() < 0.9 else 0] for _ in range(s.n_docs)] for s in segs],
                np.int64)
    W.add_field("half", [[[float(rng.uniform(1.0, 9.0))] if rng.random() < 0.7 else [] for _ in range(300)], None], np.float64)
    zed = [0.0, -0.0, 1.0, -2.0, 0.5]
    W.add_field("zed", [[[zed[int(rng.integers(0, len(zed)))]] for _ in range(s.n_docs)] for s in segs], np.float64)
    for i in range(5):
        W.add_field(f"c{i}", [[[int(rng.integers(-3, 4))] for _ in range(s.n_docs)] for s in segs], np.int64)
    W.add_filter("f0", [rng.random(s.n_docs) < 0.5 for s in segs])
    W.add_filter("f1", [rng.random(s.n_docs) < 0.5 for s in segs])
    W.rng = rng
    W.qs16 = random_queries(rng, 16, 3, 40, n_segs=2, weights=True)
    W.qs8 = random_queries(rng, 8, 3, 40, n_segs=2, weights=True)
    return W


def world_b(sa, oracle):
    rng = np.random.default_rng(23)
    n, vocab = 6000, 40
    base = random_segment(rng, n, vocab, 6)
    ends = np.array([0, 4321, n - 1], np.uint32)

    def with_ends(df):
        inner = rng.choice(np.setdiff1d(np.arange(1, n - 1), ends), size=df - len(ends), replace=False)
        return np.sort(np.concatenate([ends, inner.astype(np.uint32)])).astype(np.uint32)

    lists = {"c1": np.array([4321], np.uint32), "c63": with_ends(63), "c64": with_ends(64), "c65": with_ends(65),
             "c129": with_ends(129), "all": np.arange(n, dtype=np.uint32)}
    seg = _append_lists(base, [(d, rng.integers(1, 4, size=len(d))) for d in lists.values()])
    W = World(sa, oracle, [seg])
    W.T = {name: vocab + i for i, name in enumerate(lists)}
    rank = np.full(n, 1000, np.int64)
    rank[lists["c129"]] = np.arange(129)
    W.add_field("rank", [[[int(v)] for v in rank]], np.int64)
    W.add_field("parity", [[[float(d & 1)] for d in range(n)]], np.float64)
    for m in KEEPS:
        W.add_field(f"keep{m}", [[[1.0 if v >= 129 - m else 0.0] for v in rank]], np.float64)
    W.lists, W.rng = lists, rng
    return W


def one_term_queries(W, names):
    return csr([[(W.T[nm], 1.0 + 0.25 * i)] for i, nm in enumerate(names)], 1)
