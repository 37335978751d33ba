"""Device time of the IVF vector search (slg_vector_search_batch_ivf_device) beside the exact call
(slg_vector_search_batch_device) and the two-pass call at refine 64 (slg_vector_search_batch_approx_device), in one
process and one run, after warm-up.
Store: config 5's shape (1M x 768 f32, cosine), 1024 queries, one clause, cand_size 20, k_out 11; the rows (and the
queries) are drawn around 1024 random unit centres and re-normalised, so that lists mean something.  Centroids:
searchlite_amd.ivf.train_centroids on a 65 536-row sample, 4 iterations, 1024 lists.  nprobe in {1, 4, 16, 64}.
Per nprobe: the three calls interleaved repetition by repetition (median, min, max over --reps, each repetition timed
with its own event pair) and recall@cand_size of the IVF lists against the exact lists.  Before that, once: recall
against a second, uniformly random store of the same shape (the worst case for any partition), and the one-off
clustering time of each store.
Kernel times: run the script under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python
tools/vector_ivf_time.py --schedule DIR/schedule.json`, then `python tools/vector_ivf_time.py --parse DIR`: every
call ends with one vs_blend_kernel, so the trace splits into calls, and the schedule names each call.
--metric 1: the same rows as an L2 store (vec_metric 1).
usage (GPU box): python tools/vector_ivf_time.py [--reps N] [--rows N] [--no-uniform] [--metric 0|1] [--schedule FILE] |
--parse DIR"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--lists", type=int, default=1024)
ap.add_argument("--metric", type=int, choices=(0, 1), default=0)
ap.add_argument("--no-uniform", action="store_true", help="skip the uniformly random store")
ap.add_argument("--schedule", default=None, help="write the label of every call, in order, to this file")
ap.add_argument("--parse", default=None, help="a rocprofv3 output directory holding schedule.json")
args = ap.parse_args()
NPROBES = (1, 4, 16, 64)
REFINE = 64
KERNELS = ("vs_ivf_scan_kernel", "vs_ivf_probe_count_kernel", "vs_ivf_plan_kernel", "vs_ivf_items_kernel",
           "vs_scan_bf16_kernel", "vs_refine_kernel", "vs_select_kernel", "vs_blend_kernel", "vs_scan_kernel")

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
    calls = calls[len(calls) - len(labels):]  # (the clustering scans come before the first call)
    assert len(calls) == len(labels), (len(calls), len(labels))
    for label in dict.fromkeys(l for l in labels if not l.startswith("warm")):
        mine = [c for c, l in zip(calls, labels) if l == label]
        med = {k: float(np.median([c.get(k, 0) for c in mine])) / 1e6 for k in KERNELS}
        print(f"{label}: kernel ms per call (median of {len(mine)}): " +
              ", ".join(f"{k} {v:.3f}" for k, v in med.items() if v > 0), flush=True)
    sys.exit(0)

import torch  # noqa: E402
from searchlite_amd import corpus, ivf, searcher, _native as N  # noqa: E402
from searchlite_amd.segment import Segment  # noqa: E402

n, dim, nq, cand, k_out = args.rows, 768, 1024, 20, 11
L = N.load()
dev = torch.device("cuda", 0)
cf = np.array([0], np.uint32)
al = torch.zeros((nq, 1), dtype=torch.float32, device=dev)
schedule = []


def clustered_rows(count, centres, seed, sigma=0.02):
    """rows around the centres (centre + sigma * N(0, I), re-normalised), block by block"""
    rng = np.random.default_rng(seed)
    out = np.empty((count, dim), np.float32)
    for b in range(0, count, 65536):
        m = min(65536, count - b)
        v = centres[rng.integers(0, len(centres), m)] + sigma * rng.standard_normal((m, dim), dtype=np.float32)
        out[b:b + m] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return out


def index_of(vals):
    seg = Segment(n_docs=len(vals), term_offsets=[0, 1], doc_ids=[0], tfs=[1],
                  field_doc_len=[np.ones(len(vals), np.float32)], field_avgdl=[1.0], docs=float(len(vals)),
                  vec_dim=dim, vec_metric=args.metric, vec_offsets=np.arange(len(vals), dtype=np.uint32),
                  vec_values=vals)
    ix = searcher.GpuIndex([seg])
    ix.set_stream(torch.cuda.current_stream().cuda_stream)
    return ix


def cluster(ix, vals, what):
    t0 = time.perf_counter()
    cents = ivf.train_centroids(vals, args.lists, ivf.COSINE, iters=4, seed=0, sample=65536)
    t1 = time.perf_counter()
    ix.cluster_vector_field(0, [cents])
    t2 = time.perf_counter()
    begin, _, _ = ix.fetch_vector_lists(0, 0, dim)
    lens = np.diff(begin.astype(np.int64))
    print(f"{what}: {len(cents)} lists; train_centroids (host, 65536-row sample, 4 iterations) {t1 - t0:.2f} s; "
          f"slg_index_cluster_vector_field (assignment + list build on the device, one-off) {(t2 - t1) * 1e3:.1f} ms; "
          f"list length min {lens.min()} median {int(np.median(lens))} max {lens.max()}", flush=True)


def outputs(k):
    od = torch.empty((nq, k), dtype=torch.int32, device=dev)
    return (od, torch.empty_like(od), torch.empty((nq, k), device=dev), torch.empty((nq, k), device=dev),
            torch.empty(nq, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int64, device=dev))


def call(ix, qv, kind, arg, k, out, label):
    ptrs = [o.data_ptr() for o in out]
    head = (ix._h, nq, 1, cf.ctypes.data, qv.data_ptr(), al.data_ptr(), None, None, cand)
    if kind == "ivf":
        N.check(L.slg_vector_search_batch_ivf_device(*head, arg, k, *ptrs))
    elif kind == "approx":
        N.check(L.slg_vector_search_batch_approx_device(*head, arg, k, *ptrs))
    else:
        N.check(L.slg_vector_search_batch_device(*head, k, *ptrs))
    schedule.append(label)


def lists_of(ix, qv, kind, arg, label):
    out = outputs(cand)  # k_out = cand_size rows of the one clause's list
    call(ix, qv, kind, arg, cand, out, label)
    torch.cuda.synchronize()
    return out[0].cpu().numpy()


def recall_of(got, exact):
    return float(np.mean([len(set(got[q]) & set(exact[q])) / cand for q in range(nq)]))


centres = corpus.unit_vectors(1024, dim, seed=10)
if not args.no_uniform:
    vals = corpus.unit_vectors(n, dim, seed=21)
    ix = index_of(vals)
    cluster(ix, vals, f"uniformly random store {n} x {dim}")
    qv = torch.from_numpy(corpus.unit_vectors(nq, dim, seed=22)).to(dev)
    exact = lists_of(ix, qv, "exact", 0, "warm uniform exact lists")
    print("uniformly random store (the worst case for any partition): recall@%d " % cand +
          ", ".join(f"nprobe {p}: {recall_of(lists_of(ix, qv, 'ivf', p, 'warm uniform ivf lists'), exact):.4f}"
                    for p in NPROBES), flush=True)
    ix.close()
    del ix, vals

vals = clustered_rows(n, centres, seed=11)
ix = index_of(vals)
cluster(ix, vals, f"clustered store {n} x {dim} (rows around 1024 unit centres, sigma 0.02)")
ix.quantize_vector_field(0)
qv = torch.from_numpy(clustered_rows(nq, centres, seed=12)).to(dev)
print(f"store {n} x {dim}: f32 {n * dim * 4 / 1e9:.2f} GB; lists {n * 4 / 1e6:.1f} MB + centroids "
      f"{args.lists * dim * 4 / 1e6:.1f} MB", flush=True)


def timed(kind, arg, out, label):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call(ix, qv, kind, arg, k_out, out, label)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


exact = lists_of(ix, qv, "exact", 0, "warm exact lists")
out = outputs(k_out)
for nprobe in NPROBES:
    recall = recall_of(lists_of(ix, qv, "ivf", nprobe, "warm ivf lists"), exact)
    kinds = (("exact", 0, f"exact (beside nprobe {nprobe})"), ("approx", REFINE, f"two-pass refine {REFINE} (beside "
             f"nprobe {nprobe})"), ("ivf", nprobe, f"ivf nprobe {nprobe}"))
    for _ in range(3):  # warm-up of the three calls at the timed shape
        for kind, arg, label in kinds:
            call(ix, qv, kind, arg, k_out, out, "warm " + label)
    torch.cuda.synchronize()
    t = {kind: [] for kind, _, _ in kinds}
    for _ in range(args.reps):
        for kind, arg, label in kinds:
            t[kind].append(timed(kind, arg, out, label))
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = max(t["exact"]) - min(t["exact"])
    gain = med["ivf"] < med["exact"] - spread and med["ivf"] < med["approx"] - spread
    print(f"nprobe {nprobe}: " + ", ".join(f"{k} {med[k]:.3f} ms (min {min(t[k]):.3f}, max {max(t[k]):.3f})"
                                          for k in ("exact", "approx", "ivf")) +
          f" over {args.reps} interleaved repetitions; exact / ivf = {med['exact'] / med['ivf']:.2f}x, two-pass / ivf = "
          f"{med['approx'] / med['ivf']:.2f}x; exact spread {spread:.3f} ms; below both by more than the spread: "
          f"{'yes' if gain else 'no'}; {nq / med['ivf'] * 1e3:.0f} queries/s; recall@{cand} {recall:.4f}", flush=True)
if args.schedule:
    os.makedirs(os.path.dirname(os.path.abspath(args.schedule)), exist_ok=True)
    json.dump(schedule, open(args.schedule, "w"))
ix.close()
