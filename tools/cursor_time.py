"""Device time of cursor pages (slg_batch_prepare_after) at config 2's shape: 1M Zipf docs, 1024 queries of 3
terms, k = 11.  Page 1 (every query without a cursor) and a cursor page at rank 1 000 and at rank 10 000 (each
query's cursor = its hit at that rank; a query with fewer hits gets its last hit), in score order and for one
i64 field asc, next to the score path's own batches (k = 11: merge path; k = 1001: candidates mode, the
yardstick of profiles/sorted_time.txt).  Per batch as tools/sorted_time.py: batch_ms (HIP events around
slg_batch_run), score_ms (the scoring kernel, slg_profile_*), select_ms = the difference (partition + select).
usage (GPU box): python tools/cursor_time.py [reps]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from searchlite_amd import corpus, searcher  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
n_docs, vocab, nq, T = 1_000_000, 1 << 18, 1024, 3
seg = corpus.zipf_segment(n_docs, vocab, seed=42, n_threads=16)
offs, terms, w = corpus.zipf_queries(nq, T, seed=7, vocab=vocab)
rng = np.random.default_rng(5)
i64_vals = rng.integers(0, 1000, n_docs).astype(np.int64)
ix = searcher.GpuIndex([seg])
ix.set_stream(torch.cuda.current_stream().cuda_stream)
f_i64 = ix.add_sort_field([(np.arange(n_docs + 1, dtype=np.uint32), i64_vals)], np.int64)


def time_batch(k, sort=None, cursors=None):
    b = ix.prepare(offs, terms, w, k, searcher.Wand, sort=sort, cursors=cursors)
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
        out = dict(batch_ms=round(batch_ms, 4), score_ms=round(score_ms / max(n, 1), 4),
                   select_ms=round(batch_ms - score_ms / max(n, 1), 4))
        if cursors is not None:
            out["seen_all"] = bool(b.cursor_seen().all())
            out["mean_matched"] = round(float(b.matched_counts().mean()), 1)
        return out
    finally:
        b.close()


def cursors_at(rank, sort):
    """each query's hit at `rank` (1-based; its last hit if it has fewer) as its cursor"""
    if sort is None:
        doc, seg_, score, count = ix.search_batch(offs, terms, w, rank)
    else:
        doc, seg_, score, count, _ = ix.search_sorted(offs, terms, w, rank, sort)
    out = []
    for q in range(nq):
        c = int(count[q])
        if c == 0:
            out.append(None)
            continue
        i = min(rank, c) - 1
        d = int(doc[q, i])
        out.append(((score[q, i],) if sort is None else (int(i64_vals[d]),), int(seg_[q, i]), d))
    return out


rows = []
for k in (11, 1001):
    rows.append(dict(what="score path", k=k, **time_batch(k)))
base = rows[-1]["batch_ms"]
for name, sort in (("score order", None), ("i64 asc", [(f_i64, "asc")])):
    for rank in (0, 1000, 10000):
        cur = [None] * nq if rank == 0 else cursors_at(rank, sort)
        r = time_batch(11, sort, cur)
        rows.append(dict(what=name, page="1" if rank == 0 else f"after rank {rank}", k=11,
                         ratio_vs_score_path_k1001=round(r["batch_ms"] / base, 2), **r))
    if sort is not None:
        r = time_batch(11, sort)
        rows.append(dict(what=name, page="1 (slg_batch_prepare_sorted)", k=11,
                         ratio_vs_score_path_k1001=round(r["batch_ms"] / base, 2), **r))
for r in rows:
    print(json.dumps(r), flush=True)
