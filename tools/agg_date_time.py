"""Device time of the date_histogram and filter aggregations at the shape of tools/agg_time.py: 1M Zipf docs, 1024
queries of 3 terms, k = 11, a sorted batch (one i64 field asc).  The time the aggregations add to the batch for
(d) a root date_histogram by calendar month and (e) by calendar day over six years of timestamps (72 and 2192 rows:
the LDS home), (f) filter -> stats over a bitmap filter that half the docs pass, and, for comparison in the same
run, agg_time.py's (c) terms(1000) -> histogram(~50 buckets: the global home).  Per batch: HIP events around
slg_batch_run, mean of `reps` runs after two warm-up runs; the whole measurement is repeated `rounds` times so the
file shows the run-to-run spread.
usage (GPU box): python tools/agg_date_time.py [reps] [rounds]"""
import json
import os
import sys

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
t0, t1 = 1_546_300_800_000, 1_735_689_600_000  # 2019-01-01 .. 2025-01-01
half = ix.add_filter([rng.random(n_docs) < 0.5])
fields = {
    "x": {"id": ix.add_agg_field([csr + (rng.standard_normal(n_docs),)], np.float64)},
    "t": {"id": ix.add_agg_field([csr + (rng.integers(0, 750, n_docs).astype(np.int64),)], np.int64)},
    "ts": {"id": ix.add_agg_field([csr + (rng.integers(t0, t1, n_docs).astype(np.int64),)], np.int64)},
    "k1000": {"id": ix.add_agg_keyword_field([csr + (rng.integers(0, 1000, n_docs).astype(np.uint32),)], 1000),
              "keys": [f"k{i:04d}" for i in range(1000)]},
    A.FILTERS: lambda body: half,
}
specs = {
    "(d) root date_histogram(month)": {"h": {"type": "date_histogram", "field": "ts", "calendar_interval": "month"}},
    "(e) root date_histogram(day)": {"h": {"type": "date_histogram", "field": "ts", "calendar_interval": "day"}},
    "(f) filter -> stats": {"f": {"type": "filter", "filter": {"half": True},
                                  "aggs": {"s": {"type": "stats", "field": "x"}}}},
    "(c) terms(1000) -> histogram(50)": {"d": {"type": "terms", "field": "k1000",
                                              "aggs": {"h": {"type": "histogram", "field": "t", "interval": 15}}}},
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
            out["cells"] = sum(x["parent_rows"] * x["rows"] for x in lay)
            out["lds"] = sum(x["parent_rows"] * x["rows"] * (32 if x["is_stats"] else 4) for x in lay) <= N.AGG_LDS_BYTES
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
