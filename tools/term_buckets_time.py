"""Device time of significant_terms / rare_terms batches (slg_batch_prepare_term_buckets) at the shape of
tools/composite_time.py: 1M Zipf docs, 1024 queries of 3 terms, the i64 sort, k = 11.  Measured, each alternating with
the sorted batch without aggregations (a):
  (b) that batch with terms(3000): the yardstick, the dense table the caller copies and sorts today
  (c) significant_terms over kw3000, size 10 and size 1024, with and without a background filter, with a stats child
  (d) rare_terms over kw3000, size 10
  (e) prepare: the host time of slg_batch_prepare_term_buckets of a significant node (bg_count_kernel runs in it) next
      to that of a rare node (no background), and their difference
  (f) the substitute a caller has today for (c) and (d): the terms(3000) batch, slg_batch_fetch_aggs of the full tables
      (nq x 3000 cells) and a host sort for ten rows per query — wall clock from run to the sorted rows
Per batch: HIP events around `reps` runs after two warm-up runs; the whole measurement is repeated `rounds` times; the
last lines give the median of the rounds and their spread, and the spread of (a) itself from round to round.
usage (on a machine with the GPU): python tools/term_buckets_time.py [reps] [rounds] [base]
  base: only (a) — what runs unchanged on the parent commit, for the comparison of the two"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from searchlite_amd import aggs as A, corpus, searcher  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
base_only = len(sys.argv) > 3 and sys.argv[3] == "base"
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
    "f": {"id": ix.add_agg_field([csr + (rng.random(n_docs) * 100.0,)], np.float64)},
}
half = ix.add_filter([rng.random(n_docs) < 0.5])
fields[A.FILTERS] = lambda body: half
stats = {"s": {"type": "stats", "field": "f"}}
sig = lambda size, **more: {"g": dict({"type": "significant_terms", "field": "kw3000", "size": size}, **more)}
TERMS = {"t": {"type": "terms", "field": "kw3000"}}
specs = {} if base_only else {
    "(b) terms(3000)": TERMS,
    "(c) significant kw3000, size 10": sig(10),
    "(c) significant kw3000, size 1024": sig(1024),
    "(c) significant kw3000, size 10, background filter": sig(10, background_filter={"name": "half"}),
    "(c) significant kw3000, size 1024, background filter": sig(1024, background_filter={"name": "half"}),
    "(c) significant kw3000, size 10, stats child": sig(10, aggs=stats),
    "(c) significant kw3000, size 1024, stats child": sig(1024, aggs=stats),
    "(d) rare kw3000, size 10, max_doc_count 3": {"r": {"type": "rare_terms", "field": "kw3000", "size": 10, "max_doc_count": 3}},
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
    if base_only:
        for x in (base, base):
            x.run()
        torch.cuda.synchronize()
        for rnd in range(rounds * 4):
            base_ms.append(timed(base))
            print(json.dumps(dict(round=rnd, base_ms=round(base_ms[-1], 4))), flush=True)
    for name, request in specs.items():
        with ix.prepare(offs, terms, w, 11, searcher.Wand, sort=sort, aggs=A.agg_spec(request, fields)) as b:
            for x in (base, b, base, b):  # warm-up
                x.run()
            torch.cuda.synchronize()
            if b.term_bucket_spec is not None:
                got = b.term_buckets()["nodes"][0]
                print(json.dumps(dict(spec=name, buckets_mean=float(got["n_buckets"].mean()))), flush=True)
            for rnd in range(rounds):
                t_base, t_b = timed(base), timed(b)
                base_ms.append(t_base)
                added[name].append(t_b - t_base)
                print(json.dumps(dict(round=rnd, spec=name, base_ms=round(t_base, 4), batch_ms=round(t_b, 4),
                                      added_ms=round(t_b - t_base, 4))), flush=True)
    if not base_only:
        # (e) prepare with and without a background
        prep = {"significant": [], "rare": []}
        for rnd in range(rounds):
            for kind, request in (("significant", sig(10)), ("rare", specs["(d) rare kw3000, size 10, max_doc_count 3"])):
                plan = A.agg_spec(request, fields)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                b = ix.prepare(offs, terms, w, 11, searcher.Wand, sort=sort, aggs=plan)
                prep[kind].append((time.perf_counter() - t0) * 1e3)
                b.close()
        print(json.dumps(dict(spec="(e) prepare, host wall clock", significant_ms_median=round(statistics.median(prep["significant"]), 4),
                              rare_ms_median=round(statistics.median(prep["rare"]), 4),
                              background_ms=round(statistics.median(prep["significant"]) - statistics.median(prep["rare"]), 4),
                              significant_ms=[round(x, 3) for x in prep["significant"]],
                              rare_ms=[round(x, 3) for x in prep["rare"]])), flush=True)
        # (f) the substitute: terms(3000), the full tables to the host, ten rows per query by a host sort
        sub, sub_run = [], []
        with ix.prepare(offs, terms, w, 11, searcher.Wand, sort=sort, aggs=A.agg_spec(TERMS, fields)) as b:
            b.run()
            b.aggs()
            for rnd in range(rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                b.run()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                tab = b.aggs()[0][:, 0, :]  # [nq, 3000]
                # rare: the ten smallest counts >= 1 by (count, ordinal); the key order is the ordinal's here
                order = np.argsort(np.where(tab == 0, np.iinfo(np.int64).max, tab.astype(np.int64)), axis=1, kind="stable")[:, :10]
                rows = np.take_along_axis(tab, order, axis=1)
                sub_run.append((t1 - t0) * 1e3)
                sub.append((time.perf_counter() - t0) * 1e3)
            del rows
        print(json.dumps(dict(spec="(f) substitute: terms(3000) run + fetch of the full tables + host sort, wall clock",
                              total_ms_median=round(statistics.median(sub), 3), run_ms_median=round(statistics.median(sub_run), 3),
                              fetch_and_sort_ms_median=round(statistics.median(sub) - statistics.median(sub_run), 3),
                              total_ms=[round(x, 2) for x in sub])), flush=True)
        # the same wall clock for the device's own answer: run + slg_batch_fetch_term_buckets
        own = []
        with ix.prepare(offs, terms, w, 11, searcher.Wand, sort=sort, aggs=A.agg_spec(specs["(d) rare kw3000, size 10, max_doc_count 3"], fields)) as b:
            b.run()
            b.term_buckets()
            for rnd in range(rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                b.run()
                b.term_buckets()
                own.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps(dict(spec="(f) rare size 10: run + slg_batch_fetch_term_buckets, wall clock",
                              total_ms_median=round(statistics.median(own), 3), total_ms=[round(x, 2) for x in own])), flush=True)
finally:
    base.close()
print(json.dumps(dict(spec="(a) sorted batch without aggregations", ms_median=round(statistics.median(base_ms), 4),
                      ms_min=round(min(base_ms), 4), ms_max=round(max(base_ms), 4), samples=len(base_ms))), flush=True)
for name, xs in added.items():
    print(json.dumps(dict(spec=name, added_ms_median=round(statistics.median(xs), 4), added_ms_min=round(min(xs), 4),
                          added_ms_max=round(max(xs), 4), rounds=rounds, reps=reps)), flush=True)
