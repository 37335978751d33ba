"""Device time of field collapsing (slg_batch_prepare_collapse) at config 2's shape: 1M Zipf docs, 1024 queries of 3
terms, one keyword column of 1000 ordinals, group_limit 10, k in {11, 101, 1001, 4096}.  Per k the same batch
without the spec and with it — no inner hits, inner hits (0, 3) in the batch's order, inner hits (0, 3) under a
one-part inner sort (an i64 field asc): batch_ms = HIP events around slg_batch_run; collapse_ms = the difference to
the batch without the spec, the collapse kernel's cost; select_ms of the plain batch = batch_ms - the scoring kernel
(slg_profile_*).  Then what a caller moves to the host: fetch_rows_ms = slg_batch_fetch of the full rows at that k
(what host-side collapsing needs before it can start), fetch_collapse_ms = slg_batch_fetch_collapse.
usage (GPU box): python tools/collapse_time.py [reps]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from searchlite_amd import corpus, searcher  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
n_docs, vocab, nq, T, n_ords, G = 1_000_000, 1 << 18, 1024, 3, 1000, 10
seg = corpus.zipf_segment(n_docs, vocab, seed=42, n_threads=16)
offs, terms, w = corpus.zipf_queries(nq, T, seed=7, vocab=vocab)
rng = np.random.default_rng(5)
ords = rng.integers(0, n_ords, n_docs).astype(np.uint32)
i64_vals = rng.integers(0, 1000, n_docs).astype(np.int64)
every_doc = np.arange(n_docs + 1, dtype=np.uint32)
ix = searcher.GpuIndex([seg])
ix.set_stream(torch.cuda.current_stream().cuda_stream)
f_ord = ix.add_agg_keyword_field([(every_doc, ords)], n_ords)
f_i64 = ix.add_sort_field([(every_doc, i64_vals)], np.int64)


def host_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    return round((time.perf_counter() - t0) * 1e3 / reps, 4)


def time_batch(k, collapse=None):
    b = ix.prepare(offs, terms, w, k, searcher.Wand, collapse=collapse)
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
        out = dict(batch_ms=round(a.elapsed_time(e) / reps, 4), score_ms=round(score_ms / max(n, 1), 4))
        out["fetch_rows_ms"] = host_ms(b.fetch)
        if collapse is not None:
            out["fetch_collapse_ms"] = host_ms(b.collapse_groups)
            g = b.collapse_groups()
            out["mean_total_groups"] = round(float(g["total_groups"].mean()), 1)
            out["mean_rows"] = round(float(b.fetch()[3].mean()), 1)
        return out
    finally:
        b.close()


VARIANTS = (("no inner hits", dict()), ("inner (0, 3), batch order", dict(inner_size=3)),
            ("inner (0, 3), i64 asc", dict(inner_size=3, inner_sort=[(f_i64, "asc")])))
for k in (11, 101, 1001, 4096):
    plain = time_batch(k)
    plain["select_ms"] = round(plain["batch_ms"] - plain["score_ms"], 4)
    print(json.dumps(dict(what="without collapse", k=k, **plain)), flush=True)
    for name, extra in VARIANTS:
        r = time_batch(k, dict(field=f_ord, group_limit=min(G, k), **extra))
        print(json.dumps(dict(what=name, k=k, collapse_ms=round(r["batch_ms"] - plain["batch_ms"], 4), **r)), flush=True)
