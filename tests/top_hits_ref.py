"""The top_hits aggregation restated in plain Python (TopHitsCollector, query/aggs/mod.rs:1870-1981;
merge_top_hits, :2426-2459): the reference for tests/test_gpu_top_hits.py, itself checked against hand-derived tables
in tests/test_top_hits_ref.py.

A hit is (seg, doc, score).  A sort is [(part, order)], part = "_score" or a field name in `fields` (name ->
(values[seg][doc] = list of numbers, is_float)), as in tests/collapse_ref.py, whose SortKey restatement this uses;
an empty sort is `_score` desc.  The score a collector is handed is the request's ScoreMode's: the BM25 score, or 0.0
under a field sort without a `_score` part (the callers pass it so).

Two ways to the lists, both here:
  one_list      every hit feeds ONE collector: the limit = max(from + size, size, 1) best by SortKey are kept, the
                response is their rows [from, from + size).  This is the contract of the device
                (include/searchlite_gpu.h), which sees the candidates of all segments together.
  per_segment   the reference's own path: a collector per segment, each finished (its rows [from, from + size)),
                the finished states merged left to right by merge_top_hits, which slices at `from` AGAIN.
With from = 0 the two agree on every input (the property test of tests/test_top_hits_ref.py).  With from > 0 they
agree when one segment holds the hits and differ otherwise: the reference drops the first `from` hits of every
segment and then of the merged list (test_from_is_applied_per_segment_and_again_in_the_merge pins that by hand).
The totals agree always.

Buckets: a child node sees a doc once per parent bucket it was counted in (:905-908); which buckets those are is
tests/agg_date_ref.py's buckets_of (terms, histogram, range through agg_ref.collect; date_histogram, filter its own).
"""
import numpy as np

from tests import agg_date_ref as D
from tests import collapse_ref as R


def limit_of(frm, size):
    return max(frm + size, size, 1)  # size.saturating_add(from).max(size).max(1)


class Collector:
    """TopHitsCollector: collect() keeps the `limit` best keys (a max-heap whose worst is replaced by a better
    candidate: the kept set is the `limit` smallest keys, keys are distinct), finish() sorts and slices"""

    def __init__(self, size, frm, sort, fields):
        self.size, self.frm, self.limit = size, frm, limit_of(frm, size)
        self.key = R.sort_key(R.resolve_sort(sort), fields)
        self.kept, self.total = [], 0  # [(key, hit)]

    def collect(self, seg, doc, score):
        self.total += 1
        hit = (seg, doc, score)
        ranked = (self.key(hit), hit)
        if len(self.kept) < self.limit:
            self.kept.append(ranked)
            return
        worst = max(range(len(self.kept)), key=lambda i: self.kept[i][0])
        if ranked[0] < self.kept[worst][0]:
            self.kept[worst] = ranked

    def finish(self):
        ranked = sorted(self.kept, key=lambda kh: kh[0])
        start = min(self.frm, len(ranked))
        return {"size": self.size, "from": self.frm, "total": self.total, "hits": ranked[start:start + self.size]}


def merge_top_hits(target, incoming):
    """:2426-2459, in place: the `limit` best of both states' hits, sorted, sliced at target.from"""
    limit = limit_of(target["from"], target["size"])
    target["total"] += incoming["total"]
    kept = []
    for ranked in target["hits"] + incoming["hits"]:
        if len(kept) < limit:
            kept.append(ranked)
            continue
        worst = max(range(len(kept)), key=lambda i: kept[i][0])
        if ranked[0] < kept[worst][0]:
            kept[worst] = ranked
    kept.sort(key=lambda kh: kh[0])
    start = min(target["from"], len(kept))
    target["hits"] = kept[start:start + target["size"]]


def respond(state):
    """-> (total, [(seg, doc, score)])"""
    return state["total"], [hit for _, hit in state["hits"]]


def one_list(hits, size, frm, sort, fields):
    c = Collector(size, frm, sort, fields)
    for seg, doc, score in hits:
        c.collect(seg, doc, score)
    return respond(c.finish())


def per_segment(hits, size, frm, sort, fields):
    """a collector per segment in segment order, merged as merge_aggregation_results folds them"""
    merged = None
    for s in sorted({h[0] for h in hits}):
        c = Collector(size, frm, sort, fields)
        for seg, doc, score in hits:
            if seg == s:
                c.collect(seg, doc, score)
        st = c.finish()
        if merged is None:
            merged = st
        else:
            merge_top_hits(merged, st)
    if merged is None:
        merged = Collector(size, frm, sort, fields).finish()
    return respond(merged)


def lists_of(parent, lay, hits, columns, passes, keys_of):
    """the hits of each list of a node under `parent` (None: the root, one list): [rows][hit], in collection order.
    parent: the body of a root bucket aggregation; lay: its dict(rows, first_id)"""
    if parent is None:
        return [list(hits)]
    body = D.childless(parent)
    out = [[] for _ in range(lay["rows"])]
    for seg, doc, score in hits:
        for key, did in D.buckets_of(body, columns, passes, seg, doc):
            out[D.row_of(body, lay, key, {"id": did}, keys_of)].append((seg, doc, score))
    return out


def expected(nodes, layout, hits_per_query, columns, passes, keys_of, fields, match_only=False, collect=one_list):
    """The arrays PreparedBatch.top_hits() must return.  nodes: [dict(parent = a root bucket body or None, parent_lay =
    its dict(rows, first_id), from, size, sort)]; hits_per_query[q] = [(seg, doc, score)] every matched doc with the
    score the batch's rows carry (match_only: 0.0 instead).  -> (nodes = [dict(doc, seg, score [nq, lists, size],
    count [nq, lists])], totals = [per node [nq, lists]])"""
    nq = len(hits_per_query)
    out, totals = [], []
    for nd in nodes:
        lists = 1 if nd["parent"] is None else nd["parent_lay"]["rows"]
        size = nd["size"]
        a = dict(doc=np.zeros((nq, lists, size), np.uint32), seg=np.zeros((nq, lists, size), np.uint32),
                 score=np.zeros((nq, lists, size), np.float32), count=np.zeros((nq, lists), np.uint32))
        tot = np.zeros((nq, lists), np.uint64)
        for q, hits in enumerate(hits_per_query):
            if match_only:
                hits = [(s, d, np.float32(0.0)) for s, d, _ in hits]
            for row, lst in enumerate(lists_of(nd["parent"], nd.get("parent_lay"), hits, columns, passes, keys_of)):
                total, best = collect(lst, size, nd["from"], nd["sort"], fields)
                tot[q, row] = total
                a["count"][q, row] = len(best)
                for j, (s, d, sc) in enumerate(best):
                    a["seg"][q, row, j], a["doc"][q, row, j], a["score"][q, row, j] = s, d, sc
        out.append(a)
        totals.append(tot)
    return out, totals


def assert_same_lists(got, want, what=""):
    """tolerance 0: docs, segments and counts as they are, scores as f32 bit patterns"""
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        R.assert_same_arrays(g, w, f"{what} node {i}")
