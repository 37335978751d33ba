"""Device time of composite batches (slg_batch_prepare_composite) at the shape of tools/agg_time.py: 1M Zipf docs, 1024
queries of 3 terms, the i64 sort, k = 11.  Measured, each alternating with the sorted batch without aggregations (a):
  (b) that batch with terms(3000): the yardstick, a dense table of the same key space
  (c) composite over kw3000 alone, size 10 and size 1024
  (d) composite over kw3000 x kw3000b and over kw3000 x histogram(f, 100 ids), size 100, with and without a stats child
Per batch: HIP events around `reps` runs after two warm-up runs; the whole measurement is repeated `rounds` times; the
last lines give the median of the rounds and their spread, and the spread of (a) itself from round to round.
usage (on a machine with the GPU): python tools/composite_time.py [reps] [rounds]"""
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
sort = [(f_i64, "asc")]
keys = [f"k{i:04d}" for i in range(3000)]
fields = {
    "kw3000": {"id": ix.add_agg_keyword_field([csr + (rng.integers(0, 3000, n_docs).astype(np.uint32),)], 3000), "keys": keys},
    "kw3000b": {"id": ix.add_agg_keyword_field([csr + (rng.integers(0, 3000, n_docs).astype(np.uint32),)], 3000), "keys": keys},
    "f": {"id": ix.add_agg_field([csr + (rng.random(n_docs) * 100.0,)], np.float64)},
}
kw = {"type": "terms", "name": "a", "field": "kw3000"}
kwb = {"type": "terms", "name": "b", "field": "kw3000b"}
hist = {"type": "histogram", "name": "h", "field": "f", "interval": 1.0}
stats = {"s": {"type": "stats", "field": "f"}}
cmp = lambda sources, size, **more: {"c": dict({"type": "composite", "sources": sources, "size": size}, **more)}
specs = {
    "(b) terms(3000)": {"t": {"type": "terms", "field": "kw3000"}},
    "(c) composite kw3000, size 10": cmp([kw], 10),
    "(c) composite kw3000, size 1024": cmp([kw], 1024),
    "(d) composite kw3000 x kw3000, size 100": cmp([kw, kwb], 100),
    "(d) composite kw3000 x kw3000, size 100, stats child": cmp([kw, kwb], 100, aggs=stats),
    "(d) composite kw3000 x histogram, size 100": cmp([kw, hist], 100),
    "(d) composite kw3000 x histogram, size 100, stats child": cmp([kw, hist], 100, aggs=stats),
}


def timed(b):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        b.run()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / reps


base = ix.prepare(offs, terms, w, 11, searcher.Wand, sort=sort)
base.run()
matched = base.matched_counts()
print(json.dumps(dict(matched_mean=int(matched.mean()), matched_max=int(matched.max()))), flush=True)
added = {name: [] for name in specs}
base_ms = []
try:
    for name, request in specs.items():
        with ix.prepare(offs, terms, w, 11, searcher.Wand, sort=sort, aggs=A.agg_spec(request, fields)) as b:
            for x in (base, b, base, b):  # warm-up
                x.run()
            torch.cuda.synchronize()
            if b.composite_spec is not None:
                page = b.composite()
                print(json.dumps(dict(spec=name, buckets_mean=float(page["n_buckets"].mean()),
                                      has_more=int(page["has_more"].sum()))), flush=True)
            for rnd in range(rounds):
                t_base, t_b = timed(base), timed(b)
                base_ms.append(t_base)
                added[name].append(t_b - t_base)
                print(json.dumps(dict(round=rnd, spec=name, base_ms=round(t_base, 4), batch_ms=round(t_b, 4),
                                      added_ms=round(t_b - t_base, 4))), flush=True)
finally:
    base.close()
print(json.dumps(dict(spec="(a) sorted batch without aggregations", ms_median=round(statistics.median(base_ms), 4),
                      ms_min=round(min(base_ms), 4), ms_max=round(max(base_ms), 4), samples=len(base_ms))), flush=True)
for name, xs in added.items():
    print(json.dumps(dict(spec=name, added_ms_median=round(statistics.median(xs), 4), added_ms_min=round(min(xs), 4),
                          added_ms_max=round(max(xs), 4), rounds=rounds, reps=reps)), flush=True)
