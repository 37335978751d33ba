"""Wall time of training IVF centroids on the device (slg_index_train_vector_field: Lloyd steps over the resident f32
store) beside the host helper (searchlite_amd.ivf.train_centroids), and what the lists they leave are worth to the
IVF call.  One process, after warm-up; min .. median .. max over --reps.
Store: that of tools/vector_ivf_time.py: 1M x 768 f32, cosine, the uniformly random variant and the one drawn around
1024 random unit centres (sigma 0.02); 1024 lists.
Per store:
  device: the call's wall time (a host clock around the call, which returns after a device synchronise) at iters 4
    and 10, start = rows of the store; iters_run, empty_lists, max_len.
  host: train_centroids with the settings tools/vector_ivf_time.py records (65 536-row sample, 4 steps), repeated, and
    once on the full store with the same steps; the lists slg_index_cluster_vector_field builds around each.
  downstream (reported, not gated): the IVF call's device time and recall@20 against the exact call at nprobe 1 / 4 /
    16, over the lists of device-trained centroids (full store, 10 steps) and of the host's sample-trained centroids:
    two indexes over the same store in this process, the calls interleaved repetition by repetition.
"faster than the host helper" is said only where the medians differ by more than the larger spread (max - min) of the
two in this run.
Kernel times come from a run of their own: `rocprofv3 --kernel-trace --output-format csv -d DIR -- python
tools/vector_ivf_train_time.py --trace`, which makes one training call of 10 steps on the clustered store and nothing
else, then `python tools/vector_ivf_train_time.py --parse DIR` (append its lines to the output file).
usage (GPU box): python tools/vector_ivf_train_time.py [--reps N] [--rows N] [--out FILE] [--no-host-full]
                 | --trace | --parse DIR [--out FILE]"""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--lists", type=int, default=1024)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vsearch_ivf_train_time.txt"))
ap.add_argument("--no-host-full", action="store_true", help="skip the host helper's run over the full store")
ap.add_argument("--trace", action="store_true", help="one training call of 10 steps on the clustered store, for rocprofv3")
ap.add_argument("--parse", default=None, help="a rocprofv3 output directory of a --trace run")
args = ap.parse_args()
dim, nq, cand = 768, 1024, 20
NPROBES = (1, 4, 16)
HBM_COPY_TBS = 6.29  # MI355X: the measured float4 copy rate (8.0 TB/s spec)
KERNELS = ("vs_scan_kernel", "vs_ivf_best_kernel", "vs_ivf_moved_kernel", "vs_ivf_count_kernel",
           "vs_ivf_prefix_kernel", "vs_ivf_exscan_kernel", "vs_ivf_fill_kernel", "vs_ivf_sum_kernel",
           "vs_ivf_centroid_kernel", "vs_ivf_start_kernel")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def write_out(mode):
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, mode) as f:
        f.write("\n".join(lines) + "\n")


if args.parse:
    rows = []
    for f in glob.glob(os.path.join(args.parse, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    per = {k: [] for k in KERNELS}
    for r in rows:
        for k in KERNELS:
            if k + "<" in r["Kernel_Name"] or k + "(" in r["Kernel_Name"] or r["Kernel_Name"].endswith(k):
                per[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
                break
    say("")
    say("# kernel times: rocprofv3 --kernel-trace run of `tools/vector_ivf_train_time.py --trace` (one call, 10 steps, "
        "clustered store), --parse")
    total = sum(sum(v) for v in per.values())
    for k in KERNELS:
        v = per[k]
        if v:
            say(f"{k}: {len(v)} launches, total {sum(v):.3f} ms ({100 * sum(v) / total:.1f} % of the kernel time), "
                f"min {min(v):.3f} median {float(np.median(v)):.3f} max {max(v):.3f} ms")
    say(f"all kernels of the call: {total:.3f} ms")
    v = per["vs_ivf_sum_kernel"]
    if v:
        store = args.rows * dim * 4
        med = float(np.median(v))
        rate = store / (med * 1e-3) / 1e12
        say(f"vs_ivf_sum_kernel reads the store once per step: {store / 1e9:.3f} GB (rows x dim x 4; the doc ids and "
            f"row offsets add {args.rows * 8 / 1e6:.0f} MB, the partial sums it writes are "
            f"8 x dim bytes per (list, chunk)); at the median {med:.3f} ms that is {rate:.2f} TB/s = "
            f"{100 * rate / HBM_COPY_TBS:.0f} % of the {HBM_COPY_TBS} TB/s an f32x4 copy reaches on this part")
    write_out("a")
    sys.exit(0)

import torch  # noqa: E402
from searchlite_amd import corpus, ivf, searcher, _native as N  # noqa: E402
from searchlite_amd.segment import Segment  # noqa: E402

n = args.rows
L = N.load()
dev = torch.device("cuda", 0)
cf = np.array([0], np.uint32)


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
                  vec_dim=dim, vec_metric=0, vec_offsets=np.arange(len(vals), dtype=np.uint32), vec_values=vals)
    ix = searcher.GpuIndex([seg])
    ix.set_stream(torch.cuda.current_stream().cuda_stream)
    return ix


def mmm(t, unit="s", scale=1.0):
    return f"{min(t) * scale:.3f} .. {float(np.median(t)) * scale:.3f} .. {max(t) * scale:.3f} {unit}"


def lens_of(ix):
    begin, _, _ = ix.fetch_vector_lists(0, 0, dim)
    lens = np.diff(begin.astype(np.int64))
    return f"empty_lists {int((lens == 0).sum())}, list length min {lens.min()} median {int(np.median(lens))} max_len {lens.max()}"


def device_train(ix, iters, reps, warm):
    t, st = [], None
    for r in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = ix.train_vector_field(0, [(args.lists, iters)])[0]
        t1 = time.perf_counter()
        if r >= warm:
            t.append(t1 - t0)
    return t, st


centres = corpus.unit_vectors(1024, dim, seed=10)
if args.trace:
    vals = clustered_rows(n, centres, seed=11)
    ix = index_of(vals)
    print(ix.train_vector_field(0, [(args.lists, 10)])[0], flush=True)
    ix.close()
    sys.exit(0)

say(f"# tools/vector_ivf_train_time.py --reps {args.reps} --rows {n} --lists {args.lists} (one process; wall times "
    f"min .. median .. max over {args.reps} repetitions after warm-up)")


def host_sample(vals, reps, warm=1):
    t, cents = [], None
    for r in range(warm + reps):
        t0 = time.perf_counter()
        cents = ivf.train_centroids(vals, args.lists, ivf.COSINE, iters=4, seed=0, sample=65536)
        if r >= warm:
            t.append(time.perf_counter() - t0)
    return t, cents


def outputs(k):
    od = torch.empty((nq, k), dtype=torch.int32, device=dev)
    return (od, torch.empty_like(od), torch.empty((nq, k), device=dev), torch.empty((nq, k), device=dev),
            torch.empty(nq, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int64, device=dev))


def search(ix, qv, al, nprobe, out):
    """nprobe 0: the exact call"""
    head = (ix._h, nq, 1, cf.ctypes.data, qv.data_ptr(), al.data_ptr(), None, None, cand)
    ptrs = [o.data_ptr() for o in out]
    if nprobe:
        N.check(L.slg_vector_search_batch_ivf_device(*head, nprobe, cand, *ptrs))
    else:
        N.check(L.slg_vector_search_batch_device(*head, cand, *ptrs))


def timed(ix, qv, al, nprobe, out):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    search(ix, qv, al, nprobe, out)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def recall_of(got, exact):
    return float(np.mean([len(set(got[q]) & set(exact[q])) / cand for q in range(nq)]))


def one_store(what, vals, qv_host):
    say(f"{what}: {n} x {dim} f32 = {n * dim * 4 / 1e9:.2f} GB, cosine, {args.lists} lists")
    ix_dev, ix_host = index_of(vals), index_of(vals)
    # ---- the device call ----
    dev_t = {}
    for iters in (4, 10):
        t, st = device_train(ix_dev, iters, args.reps, warm=2)
        dev_t[iters] = t
        say(f"  device, slg_index_train_vector_field iters {iters} (full store, start = rows of the store, the final "
            f"assignment and list build included): {mmm(t)}; iters_run {st['iters_run']}, moved {st['moved']}, "
            f"empty_lists {st['empty_lists']}, max_len {st['max_len']}; {lens_of(ix_dev)}")
    # ---- the host helper ----
    t_host, cents = host_sample(vals, args.reps)
    t0 = time.perf_counter()
    ix_host.cluster_vector_field(0, [cents])
    t_cl = time.perf_counter() - t0
    say(f"  host, ivf.train_centroids (65536-row sample, 4 steps, numpy): {mmm(t_host)}; iters_run 4; then "
        f"slg_index_cluster_vector_field {t_cl * 1e3:.1f} ms; {lens_of(ix_host)}")
    for iters in (4, 10):
        a, b = dev_t[iters], t_host
        spread = max(max(a) - min(a), max(b) - min(b))
        diff = float(np.median(b)) - float(np.median(a))
        verdict = "faster than the host helper" if diff > spread else \
            ("slower than the host helper" if -diff > spread else "no faster than the host helper (within the spread)")
        say(f"  device iters {iters} (full store) against the host's sample run: medians {float(np.median(a)):.3f} s and "
            f"{float(np.median(b)):.3f} s, larger spread {spread:.3f} s: the device call is {verdict}")
    if not args.no_host_full:
        t0 = time.perf_counter()
        full = ivf.train_centroids(vals, args.lists, ivf.COSINE, iters=4, seed=0)
        t_full = time.perf_counter() - t0
        with index_of(vals) as ix_full:
            ix_full.cluster_vector_field(0, [full])
            say(f"  host, ivf.train_centroids on the full store (4 steps, once): {t_full:.2f} s; iters_run 4; "
                f"{lens_of(ix_full)}")
    # ---- downstream: the IVF call over the two sets of lists, interleaved ----
    qv = torch.from_numpy(qv_host).to(dev)
    al = torch.zeros((nq, 1), dtype=torch.float32, device=dev)
    out = outputs(cand)
    search(ix_dev, qv, al, 0, out)
    torch.cuda.synchronize()
    exact = out[0].cpu().numpy()
    for nprobe in NPROBES:
        rec = {}
        for name, ix in (("device-trained", ix_dev), ("host-sample-trained", ix_host)):
            for _ in range(3):
                search(ix, qv, al, nprobe, out)
            torch.cuda.synchronize()
            rec[name] = recall_of(out[0].cpu().numpy(), exact)
        t = {"device-trained": [], "host-sample-trained": []}
        for _ in range(max(args.reps, 10)):
            for name, ix in (("device-trained", ix_dev), ("host-sample-trained", ix_host)):
                t[name].append(timed(ix, qv, al, nprobe, out))
        say(f"  IVF call, nprobe {nprobe}, {nq} queries, cand_size {cand}, interleaved: " +
            "; ".join(f"{name} lists {mmm(t[name], 'ms')}, recall@{cand} {rec[name]:.4f}" for name in t))
    ix_dev.close()
    ix_host.close()


one_store("uniformly random store", corpus.unit_vectors(n, dim, seed=21), corpus.unit_vectors(nq, dim, seed=22))
one_store("clustered store (rows around 1024 unit centres, sigma 0.02)", clustered_rows(n, centres, seed=11),
          clustered_rows(nq, centres, seed=12))
write_out("w")
