"""Device time of the two-pass vector search (slg_vector_search_batch_approx_device) beside the exact call
(slg_vector_search_batch_device), in one process and one run, after warm-up.
Store: config 5's (1M x 768 f32, cosine), 1024 queries, one clause, cand_size 20, k_out 11; refine in {20, 32, 64, 256}.
Per refine: the exact call and the approx call interleaved repetition by repetition (median, min, max over --reps,
each repetition timed with its own event pair), and recall@cand_size of the approx lists against the exact lists.
Kernel times: run the script under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python
tools/vector_approx_time.py --schedule DIR/schedule.json`, then `python tools/vector_approx_time.py --parse DIR`:
every call ends with one vs_blend_kernel, so the trace splits into calls, and the schedule names each call.
usage (GPU box): python tools/vector_approx_time.py [--reps N] [--rows N] [--schedule FILE] | --parse DIR"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--schedule", default=None, help="write the label of every call, in order, to this file")
ap.add_argument("--parse", default=None, help="a rocprofv3 output directory holding schedule.json")
args = ap.parse_args()
REFINES = (20, 32, 64, 256)
KERNELS = ("vs_scan_bf16_kernel", "vs_refine_kernel", "vs_select_kernel", "vs_blend_kernel", "vs_scan_kernel")

if args.parse:
    labels = json.load(open(os.path.join(args.parse, "schedule.json")))
    rows = []
    for f in glob.glob(os.path.join(args.parse, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows = [r for r in rows if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], {}
    for r in rows:
        name = next(k for k in KERNELS if k + "<" in r["Kernel_Name"] or k + "(" in r["Kernel_Name"] or
                    r["Kernel_Name"].endswith(k))
        cur[name] = cur.get(name, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if name == "vs_blend_kernel":
            calls.append(cur)
            cur = {}
    assert len(calls) == len(labels), (len(calls), len(labels))
    for label in dict.fromkeys(l for l in labels if not l.startswith("warm")):
        mine = [c for c, l in zip(calls, labels) if l == label]
        med = {k: float(np.median([c.get(k, 0) for c in mine])) / 1e6 for k in KERNELS}
        print(f"{label}: kernel ms per call (median of {len(mine)}): " +
              ", ".join(f"{k} {v:.3f}" for k, v in med.items() if v > 0), flush=True)
    sys.exit(0)

import torch  # noqa: E402
from searchlite_amd import corpus, searcher, _native as N  # noqa: E402
from searchlite_amd.segment import Segment  # noqa: E402

n, dim, nq, cand, k_out = args.rows, 768, 1024, 20, 11
vals = corpus.unit_vectors(n, dim, seed=11)
seg = Segment(n_docs=n, term_offsets=[0, 1], doc_ids=[0], tfs=[1], field_doc_len=[np.ones(n, np.float32)],
              field_avgdl=[1.0], docs=float(n), vec_dim=dim, vec_metric=0,
              vec_offsets=np.arange(n, dtype=np.uint32), vec_values=vals)
ix = searcher.GpuIndex([seg])
L = N.load()
dev = torch.device("cuda", 0)
ix.quantize_vector_field(0)
bits, _ = ix.fetch_vector_copy(0, 0, dim)
print(f"store {n} x {dim}: f32 {n * dim * 4 / 1e9:.2f} GB, bf16 copy {bits.nbytes / 1e9:.2f} GB + norms "
      f"{n * 4 / 1e6:.1f} MB", flush=True)
del bits

cf = np.array([0], np.uint32)
qv = torch.from_numpy(corpus.unit_vectors(nq, dim, seed=12)).to(dev)
al = torch.zeros((nq, 1), dtype=torch.float32, device=dev)
schedule = []


def outputs(k):
    od = torch.empty((nq, k), dtype=torch.int32, device=dev)
    return (od, torch.empty_like(od), torch.empty((nq, k), device=dev), torch.empty((nq, k), device=dev),
            torch.empty(nq, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int64, device=dev))


def call(refine, k, out, label):
    ptrs = [o.data_ptr() for o in out]
    if refine:
        N.check(L.slg_vector_search_batch_approx_device(ix._h, nq, 1, cf.ctypes.data, qv.data_ptr(), al.data_ptr(), None,
                                                        None, cand, refine, k, *ptrs))
    else:
        N.check(L.slg_vector_search_batch_device(ix._h, nq, 1, cf.ctypes.data, qv.data_ptr(), al.data_ptr(), None,
                                                 None, cand, k, *ptrs))
    schedule.append(label)


def timed(refine, out, label):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call(refine, k_out, out, label)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


ix.set_stream(torch.cuda.current_stream().cuda_stream)
# the exact lists (cand_size docs per query): k_out = cand_size rows of the one clause's list
ex = outputs(cand)
call(0, cand, ex, "warm exact lists")
torch.cuda.synchronize()
exact_docs = ex[0].cpu().numpy()
out = outputs(k_out)
for refine in REFINES:
    ap_ = outputs(cand)
    call(refine, cand, ap_, "warm approx lists")
    torch.cuda.synchronize()
    got = ap_[0].cpu().numpy()
    recall = np.mean([len(set(got[q]) & set(exact_docs[q])) / cand for q in range(nq)])
    for _ in range(3):  # warm-up of both calls at the timed shape
        call(0, k_out, out, "warm exact")
        call(refine, k_out, out, "warm approx")
    torch.cuda.synchronize()
    te, ta = [], []
    for _ in range(args.reps):
        te.append(timed(0, out, f"exact (beside refine {refine})"))
        ta.append(timed(refine, out, f"approx refine {refine}"))
    me, ma = float(np.median(te)), float(np.median(ta))
    print(f"refine {refine}: exact {me:.3f} ms (min {min(te):.3f}, max {max(te):.3f}), approx {ma:.3f} ms "
          f"(min {min(ta):.3f}, max {max(ta):.3f}) over {args.reps} interleaved repetitions; exact / approx = "
          f"{me / ma:.2f}x; margin {me - ma:.3f} ms vs exact spread {max(te) - min(te):.3f} ms; "
          f"{nq / ma * 1e3:.0f} queries/s; recall@{cand} {recall:.4f}", flush=True)
if args.schedule:
    os.makedirs(os.path.dirname(os.path.abspath(args.schedule)), exist_ok=True)
    json.dump(schedule, open(args.schedule, "w"))
ix.close()
