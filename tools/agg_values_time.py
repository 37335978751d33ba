"""Device time of the value nodes (cardinality, percentiles, percentile_ranks) at the shape of tools/agg_time.py:
1M Zipf docs, 1024 queries of 3 terms, k = 11, one value per doc.  The sorted batch (one i64 field asc) without
aggregations, and the time each case adds to it:
  (d) root cardinality over a column of ~10^6 distinct values (the bitmaps in device memory: global atomicOr)
  (e) terms(8) -> cardinality over ~10^4 distinct values (the bitmaps in LDS)
  (f) root percentiles, the default percents, over the ~10^6-value column (two candidate walks, fine tables in LDS)
  (g) root percentile_ranks with 4 targets
Per batch: HIP events around slg_batch_run, mean of `reps` runs after two warm-up runs; the whole measurement is
repeated `rounds` times so the file shows the run-to-run spread.  Also the host time of slg_index_rank_agg_field.
usage (GPU box): python tools/agg_values_time.py [reps] [rounds]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from searchlite_amd import aggs as A, corpus, searcher, _native as N  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
n_docs, vocab, nq, T = 1_000_000, 1 << 18, 1024, 3
seg = corpus.zipf_segment(n_docs, vocab, seed=42, n_threads=16)
offs, terms, w = corpus.zipf_queries(nq, T, seed=7, vocab=vocab)
rng = np.random.default_rng(5)
csr = (np.arange(n_docs + 1, dtype=np.uint32),)
ix = searcher.GpuIndex([seg])
ix.set_stream(torch.cuda.current_stream().cuda_stream)
f_i64 = ix.add_sort_field([csr + (rng.integers(0, 1000, n_docs).astype(np.int64),)], np.int64)
sort = [(f_i64, "asc")]
fields = {
    "x": {"id": ix.add_agg_field([csr + (rng.standard_normal(n_docs),)], np.float64)},
    "t": {"id": ix.add_agg_field([csr + (rng.integers(0, 10_000, n_docs).astype(np.int64),)], np.int64)},
    "k8": {"id": ix.add_agg_keyword_field([csr + (rng.integers(0, 8, n_docs).astype(np.uint32),)], 8),
           "keys": [f"k{i}" for i in range(8)]},
}
for name in ("x", "t"):
    t0 = time.perf_counter()
    r = ix.rank_agg_field(fields[name]["id"])
    print(json.dumps(dict(rank_agg_field=name, values=n_docs, distinct=r, host_ms=round((time.perf_counter() - t0) * 1e3, 1))),
          flush=True)
specs = {
    "(d) root cardinality, ~1e6 distinct": {"c": {"type": "cardinality", "field": "x"}},
    "(e) terms(8) -> cardinality, ~1e4 distinct": {"d": {"type": "terms", "field": "k8",
                                                         "aggs": {"c": {"type": "cardinality", "field": "t"}}}},
    "(f) root percentiles, default percents, ~1e6 distinct": {"p": {"type": "percentiles", "field": "x"}},
    "(g) root percentile_ranks, 4 targets": {"r": {"type": "percentile_ranks", "field": "x",
                                                  "values": [-1.0, 0.0, 0.5, 2.0]}},
}


def time_batch(aggs):
    kw = {} if aggs is None else {"aggs": A.agg_spec(aggs, fields)}
    b = ix.prepare(offs, terms, w, 11, searcher.Wand, sort=sort, **kw)
    try:
        for _ in range(2):
            b.run()
        torch.cuda.synchronize()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            b.run()
        e.record()
        torch.cuda.synchronize()
        matched = b.matched_counts()
        out = dict(batch_ms=round(a.elapsed_time(e) / reps, 4), matched_mean=int(matched.mean()),
                   matched_max=int(matched.max()))
        if aggs is not None:
            lay = b.agg_layout()
            out["value_cells"] = sum(x["parent_rows"] * x["rows"] for x in lay if x["is_values"])
        return out
    finally:
        b.close()


for rnd in range(rounds):
    base = time_batch(None)
    print(json.dumps(dict(round=rnd, spec="sorted batch, i64 asc, no aggregations", **base)), flush=True)
    for name, req in specs.items():
        r = time_batch(req)
        print(json.dumps(dict(round=rnd, spec=name, added_ms=round(r["batch_ms"] - base["batch_ms"], 4), **r)),
              flush=True)
