"""Device time of field-sorted batches (slg_batch_prepare_sorted) at config 2's shape: 1M Zipf docs, 1024
queries of 3 terms, k = 11 and 1001, for three sort specs — one i64 field asc; an f64 field desc + _score
desc; a field of 8 distinct values (asc) — next to the same queries on the `_score` path at k = 1001
(candidates mode too: the yardstick).  Per batch: the scoring kernel's time (slg_profile_* events) and the
whole batch (partition + score + select, HIP events around slg_batch_run); their difference is the
partition and select kernels (select_topk_kernel / select_sorted_kernel).
usage (GPU box): python tools/sorted_time.py [reps]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from searchlite_amd import corpus, searcher, _native as N  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
n_docs, vocab, nq, T = 1_000_000, 1 << 18, 1024, 3
seg = corpus.zipf_segment(n_docs, vocab, seed=42, n_threads=16)
offs, terms, w = corpus.zipf_queries(nq, T, seed=7, vocab=vocab)
rng = np.random.default_rng(5)
csr = (np.arange(n_docs + 1, dtype=np.uint32),)
L = N.load()
ix = searcher.GpuIndex([seg])
ix.set_stream(torch.cuda.current_stream().cuda_stream)
f_i64 = ix.add_sort_field([csr + (rng.integers(0, 1000, n_docs).astype(np.int64),)], np.int64)
f_f64 = ix.add_sort_field([csr + (rng.standard_normal(n_docs),)], np.float64)
f_low = ix.add_sort_field([csr + (rng.integers(0, 8, n_docs).astype(np.int64),)], np.int64)


def time_batch(k, sort):
    b = ix.prepare(offs, terms, w, k, searcher.Wand, sort=sort)
    try:
        for _ in range(2):
            b.run()
        torch.cuda.synchronize()
        ix.profile(True)
        ix.profile_read()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            b.run()
        e.record()
        torch.cuda.synchronize()
        n, score_ms = ix.profile_read()
        ix.profile(False)
        batch_ms = a.elapsed_time(e) / reps
        n_post = b.info()["n_postings"]
        return dict(batch_ms=round(batch_ms, 4), score_ms=round(score_ms / max(n, 1), 4),
                    select_ms=round(batch_ms - score_ms / max(n, 1), 4), postings=int(n_post))
    finally:
        b.close()


rows = []
base = time_batch(1001, None)
rows.append(dict(spec="_score desc (score path)", k=1001, **base))
for name, sort in (("i64 asc", [(f_i64, "asc")]),
                   ("f64 desc, _score desc", [(f_f64, "desc"), ("_score", "desc")]),
                   ("8-value field asc", [(f_low, "asc")])):
    for k in (11, 1001):
        r = time_batch(k, sort)
        rows.append(dict(spec=name, k=k, ratio_vs_score_k1001=round(r["batch_ms"] / base["batch_ms"], 2), **r))
for r in rows:
    print(json.dumps(r), flush=True)
