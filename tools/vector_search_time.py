"""Device time of the exact vector-only search (slg_vector_search_batch_device) after warm-up.
Headline: config 5's store (1M x 768 f32, cosine), 1024 queries, one clause, cand_size 20, k_out 11.
Large path: cand_size 1000 over two clauses (the 768-d field and a 256-d field), k_out 1001.
Scan-kernel time comes from a rocprofv3 --kernel-trace --stats run of this script (vs_scan_kernel rows).
--metric 1: the same rows as an L2 store (vec_metric 1).
usage (GPU box): python tools/vector_search_time.py [--shape headline|large|both] [--iters N] [--metric 0|1]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from searchlite_amd import corpus, searcher, _native as N  # noqa: E402
from searchlite_amd.segment import Segment  # noqa: E402

PEAK_F32_MFMA_TF = 157.3

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="both")
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--metric", type=int, choices=(0, 1), default=0)
args = ap.parse_args()

n, dim, nq = 1_000_000, 768, 1024
vals = corpus.unit_vectors(n, dim, seed=11)
seg = Segment(n_docs=n, term_offsets=[0, 1], doc_ids=[0], tfs=[1], field_doc_len=[np.ones(n, np.float32)],
              field_avgdl=[1.0], docs=float(n), vec_dim=dim, vec_metric=args.metric,
              vec_offsets=np.arange(n, dtype=np.uint32), vec_values=vals)
ix = searcher.GpuIndex([seg])
L = N.load()
dev = torch.device("cuda", 0)


def timed(label, clause_field, qv, cand, k_out):
    nc = len(clause_field)
    cf = np.array(clause_field, np.uint32)
    al = torch.zeros((nq, nc), dtype=torch.float32, device=dev)
    od = torch.empty((nq, k_out), dtype=torch.int32, device=dev)
    os_, osc, ov = torch.empty_like(od), torch.empty((nq, k_out), device=dev), torch.empty((nq, k_out), device=dev)
    oc = torch.empty(nq, dtype=torch.int32, device=dev)
    ot = torch.empty(nq, dtype=torch.int64, device=dev)

    def run():
        N.check(L.slg_vector_search_batch_device(ix._h, nq, nc, cf.ctypes.data, qv.data_ptr(), al.data_ptr(), None,
                                                 None, cand, k_out, od.data_ptr(), os_.data_ptr(), osc.data_ptr(),
                                                 ov.data_ptr(), oc.data_ptr(), ot.data_ptr()))
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    ix.set_stream(torch.cuda.current_stream().cuda_stream)
    run()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        run()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / args.iters
    dims = sum(dim if f == 0 else 256 for f in clause_field)
    flop = 2.0 * nq * n * dims
    print(f"{label}: {ms:.3f} ms per batch of {nq} queries, {nq / ms * 1e3:.0f} queries/s, "
          f"whole-call {flop / ms / 1e9:.1f} TFLOP/s ({flop / ms / 1e9 / PEAK_F32_MFMA_TF * 100:.1f} % of the "
          f"{PEAK_F32_MFMA_TF} TF f32 matrix peak); store bytes {n * dims * 4 / 1e9:.2f} GB", flush=True)


if args.shape in ("headline", "both"):
    qv = torch.from_numpy(corpus.unit_vectors(nq, dim, seed=12)).to(dev)
    timed("headline 1M x 768 cosine, 1 clause, cand 20, k_out 11", [0], qv, 20, 11)
if args.shape in ("large", "both"):
    f1 = ix.add_vector_field([(args.metric, np.arange(n, dtype=np.uint32), corpus.unit_vectors(n, 256, seed=31))])
    qv = torch.from_numpy(np.concatenate([corpus.unit_vectors(nq, dim, seed=12), corpus.unit_vectors(nq, 256, seed=13)],
                                         axis=1)).to(dev)
    timed("large path 2 clauses (768-d + 256-d), cand 1000, k_out 1001", [0, f1], qv, 1000, 1001)
ix.close()
