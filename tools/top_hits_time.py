"""Device time of top_hits batches (slg_batch_prepare_top_hits) at the shape of tools/agg_time.py: 1M Zipf docs, 1024
queries of 3 terms, the i64 sort, k = 11.  For (a) terms(8) with top_hits size 3, (b) terms(1000) with top_hits size 3
and (c) a root top_hits size 10 with a field sort: slg_batch_run of the batch with the spec and of the same batch
without it (an aggregation batch for (a) and (b), the sorted batch for (c): what the parent commit runs), the two
alternating.  The difference is the kernel's cost.  Per batch: HIP events around `reps` runs after two warm-up runs;
the whole measurement is repeated `rounds` times; the last lines give the median of the rounds and their spread.
max_entries is set to what the largest query needs (the column is single-valued: its matched docs), so the run
scratch is 8 B x max_entries x 1024 queries.
usage (GPU box): python tools/top_hits_time.py [reps] [rounds]"""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from searchlite_amd import aggs as A, corpus, searcher  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n_docs, vocab, nq, T = 1_000_000, 1 << 18, 1024, 3
seg = corpus.zipf_segment(n_docs, vocab, seed=42, n_threads=16)
offs, terms, w = corpus.zipf_queries(nq, T, seed=7, vocab=vocab)
rng = np.random.default_rng(5)
csr = (np.arange(n_docs + 1, dtype=np.uint32),)
ix = searcher.GpuIndex([seg])
ix.set_stream(torch.cuda.current_stream().cuda_stream)
f_i64 = ix.add_sort_field([csr + (rng.integers(0, 1000, n_docs).astype(np.int64),)], np.int64)
f_t = ix.add_sort_field([csr + (rng.integers(0, 750, n_docs).astype(np.int64),)], np.int64)
sort = [(f_i64, "asc")]
fields = {
    "t": {"sort_id": f_t},
    "k8": {"id": ix.add_agg_keyword_field([csr + (rng.integers(0, 8, n_docs).astype(np.uint32),)], 8),
           "keys": [f"k{i}" for i in range(8)]},
    "k1000": {"id": ix.add_agg_keyword_field([csr + (rng.integers(0, 1000, n_docs).astype(np.uint32),)], 1000),
              "keys": [f"k{i:04d}" for i in range(1000)]},
}
hits3 = {"type": "top_hits", "size": 3, "sort": [{"field": "t", "order": "asc"}]}
specs = {
    "(a) terms(8) -> top_hits(3)": {"d": {"type": "terms", "field": "k8", "aggs": {"best": hits3}}},
    "(b) terms(1000) -> top_hits(3)": {"d": {"type": "terms", "field": "k1000", "aggs": {"best": hits3}}},
    "(c) root top_hits(10), field sort": {"best": {"type": "top_hits", "size": 10, "sort": [{"field": "t", "order": "asc"}]}},
    # two nodes under one parent share its runs: what the second adds is one more select, the rest of (a) / (b) is
    # the offsets and the fill
    "(a2) terms(8) -> 2 x top_hits(3)": {"d": {"type": "terms", "field": "k8", "aggs": {"best": hits3, "more": hits3}}},
    "(b2) terms(1000) -> 2 x top_hits(3)": {"d": {"type": "terms", "field": "k1000", "aggs": {"best": hits3, "more": hits3}}},
}


def prepared(request, with_hits, max_entries):
    plan = A.agg_spec(request, fields, top_hits_max_entries=max_entries)
    if with_hits:
        return ix.prepare(offs, terms, w, 11, searcher.Wand, sort=sort, aggs=plan)
    if plan.spec.n_nodes:
        return ix.prepare(offs, terms, w, 11, searcher.Wand, sort=sort, aggs=plan.spec)
    return ix.prepare(offs, terms, w, 11, searcher.Wand, sort=sort)


def timed(b):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        b.run()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / reps


with ix.prepare(offs, terms, w, 11, searcher.Wand, sort=sort) as b0:
    b0.run()
    matched = b0.matched_counts()
max_entries = int(matched.max())
print(json.dumps(dict(matched_mean=int(matched.mean()), matched_max=max_entries, max_entries=max_entries,
                      run_scratch_mb=round(8 * max_entries * nq / 2 ** 20, 1))), flush=True)
added = {name: [] for name in specs}
for name, request in specs.items():
    base, hits = prepared(request, False, max_entries), prepared(request, True, max_entries)
    try:
        for b in (base, hits, base, hits):  # warm-up
            b.run()
        torch.cuda.synchronize()
        assert not hits.top_hits()["status"].any()
        for rnd in range(rounds):
            t_base, t_hits = timed(base), timed(hits)
            added[name].append(t_hits - t_base)
            print(json.dumps(dict(round=rnd, spec=name, base_ms=round(t_base, 4), top_hits_ms=round(t_hits, 4),
                                  added_ms=round(t_hits - t_base, 4))), flush=True)
    finally:
        base.close()
        hits.close()
for name, xs in added.items():
    print(json.dumps(dict(spec=name, added_ms_median=round(statistics.median(xs), 4), added_ms_min=round(min(xs), 4),
                          added_ms_max=round(max(xs), 4), rounds=rounds, reps=reps)), flush=True)
