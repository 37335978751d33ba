"""Device time of the hybrid text + vector search (slg_batch_prepare_hybrid -> slg_batch_run ->
slg_batch_hybrid_device) after warm-up, on config 5's store: 1M docs x 768 f32 (cosine), 1024 three-term
queries, k = 1001, cand_size 1000, k_out 11; and a selective shape (rare terms: few matched docs per query).

Without --child this is the driver: every GPU step is a child process under its own `timeout`, and the first
failure stops the run.  Steps: (1) the timing child per shape (events around run = score + select and around
hybrid = gather + fold + blend; the rows the gather reads -> bytes/s; slg_batch_rerank_device of the same
batch's BM25 hits on the same store -> rerank_kernel's bytes/s), (2) per shape one rocprofv3 --kernel-trace --stats
run of the child, a run of its own, whose per-kernel table gives the split into score, select, gather, fold and
blend and the gather's bytes/s, for each shape.  Output: profiles/hybrid_time.txt (with the splits appended) and
profiles/hybrid_kernel_stats.txt.
usage (GPU box): python tools/hybrid_time.py [--iters N] [--step-timeout S]"""
import argparse
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--child", default=None, help="dense | selective (internal)")
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--step-timeout", type=int, default=420)
args = ap.parse_args()

SHAPES = {"dense": (64, 8192), "selective": (60000, 200000)}  # term rank ranges of the queries


def child(shape):
    import numpy as np
    import torch
    from searchlite_amd import corpus, searcher, _native as N
    n, vocab, dim, nq, k, cand, k_out = 1_000_000, 1 << 18, 768, 1024, 1001, 1000, 11
    seg = corpus.zipf_segment(n, vocab, seed=42, n_threads=16)
    seg.vec_dim, seg.vec_metric = dim, 0
    seg.vec_offsets = np.arange(n, dtype=np.uint32)
    seg.vec_values = corpus.unit_vectors(n, dim, seed=11)
    lo, hi = SHAPES[shape]
    offs, terms, w = corpus.zipf_queries(nq, 3, rank_lo=lo, rank_hi=hi, seed=7, vocab=vocab)
    dev = torch.device("cuda", 0)
    L = N.load()
    with searcher.GpuIndex([seg]) as ix:
        ix.set_stream(torch.cuda.current_stream().cuda_stream)
        qv = torch.from_numpy(corpus.unit_vectors(nq, dim, seed=12)).to(dev)
        al = torch.full((nq, 1), 0.5, dtype=torch.float32, device=dev)
        od = torch.empty((nq, k_out), dtype=torch.int32, device=dev)
        os_, osc, ov = torch.empty_like(od), torch.empty((nq, k_out), device=dev), torch.empty((nq, k_out), device=dev)
        oc = torch.empty(nq, dtype=torch.int32, device=dev)
        ot = torch.empty(nq, dtype=torch.int64, device=dev)
        cf = np.array([0], np.uint32)
        b = ix.prepare(offs, terms, w, k, hybrid=True)

        def hybrid():
            b.hybrid_device(cf, qv.data_ptr(), al.data_ptr(), None, cand, k_out, od.data_ptr(), os_.data_ptr(),
                            osc.data_ptr(), ov.data_ptr(), oc.data_ptr(), ot.data_ptr())

        def rerank():
            b.rerank_device(1, qv.data_ptr(), al.data_ptr(), None, k_out, od.data_ptr(), os_.data_ptr(),
                            osc.data_ptr(), ov.data_ptr(), oc.data_ptr())

        def timed(f):
            f()
            torch.cuda.synchronize()
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                f()
            e.record()
            torch.cuda.synchronize()
            return a.elapsed_time(e) / args.iters

        run_ms = timed(b.run)
        hy_ms = timed(hybrid)
        rr_ms = timed(rerank)
        # every matched doc has a vector here: the gather reads one row per matched doc
        matched = int(ot.sum().item())  # (union sizes: reported only)
        hits = int(b.fetch()[3].sum())  # the batch's BM25 hits: the rows the rerank reads
        b.close()
        with ix.prepare(offs, terms, w, 11, sort=[(N.SORT_SCORE, N.ORDER_DESC)]) as sb:
            sb.run()
            rows = int(sb.matched_counts().sum())
    gb = rows * dim * 4 / 1e9
    print(f"{shape}: 1M x 768 cosine, {nq} three-term queries (term ranks {lo}..{hi}), k {k}, cand_size {cand}, "
          f"k_out {k_out}")
    print(f"  matched docs (rows the gather reads): {rows} = {gb:.2f} GB; union sizes sum to {matched}")
    print(f"  score + select (slg_batch_run):               {run_ms:8.3f} ms per batch")
    print(f"  gather + fold + blend (slg_batch_hybrid_device): {hy_ms:8.3f} ms per batch")
    print(f"  gather rate if the whole call were the gather: {gb / hy_ms * 1e3:.1f} GB/s (a lower bound; the kernel "
          f"split below has the gather's own)")
    print(f"  rerank of the batch's {hits} BM25 hits (slg_batch_rerank_device, rerank_kernel): {rr_ms:.3f} ms = "
          f"{hits * dim * 4 / 1e9 / rr_ms * 1e3:.1f} GB/s", flush=True)


def kernel_split(shape, csv_path, rows, hits, dim=768):
    """the per-batch split of one shape from rocprofv3's kernel statistics (Name, Calls, TotalDurationNs), with the
    gather's and the rerank's rate of row reads (rows * dim * 4 bytes over the kernel's mean time)"""
    import csv
    stat = {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(csv_path))}
    pick = lambda key: next(((c, t) for n, (c, t) in stat.items() if key in n), (0, 0.0))
    (gc, gt), (fc, ft), (bc, bt) = pick("hy_gather_kernel"), pick("vs_select_kernel"), pick("vs_blend_kernel<true>")
    (sc, st), (tc, tt), (rc, rt) = pick("score_uniform4_kernel"), pick("select_topk_kernel<false>"), pick("rerank_kernel")
    per = lambda c, t: t / max(c, 1) / 1e6
    rate = lambda n, ms: n * dim * 4 / 1e9 / ms * 1e3 if ms > 0 else 0.0
    out = [f"{shape} shape, per batch, from rocprofv3 --kernel-trace --stats (mean over the calls of the run):",
           f"  score  (score_uniform4_kernel)        {per(sc, st):8.3f} ms",
           f"  select (select_topk_kernel<false>)    {per(tc, tt):8.3f} ms",
           f"  gather (hy_gather_kernel)             {per(gc, gt):8.3f} ms = {rate(rows, per(gc, gt)):.1f} GB/s of "
           f"row reads ({rows} rows)",
           f"  fold   (vs_select_kernel, {fc // max(gc, 1)} passes)   {ft / max(gc, 1) / 1e6:8.3f} ms",
           f"  blend  (vs_blend_kernel<true>)        {per(bc, bt):8.3f} ms",
           f"  rerank_kernel on the same store       {per(rc, rt):8.3f} ms = {rate(hits, per(rc, rt)):.1f} GB/s of "
           f"row reads ({hits} rows)"]
    return "\n".join(out) + "\n"


def step(cmd, log):
    print("+", " ".join(cmd), flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(args.step_timeout)] + cmd, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    log.write(r.stdout)
    log.flush()
    if r.returncode != 0:
        print(r.stdout[-2000:])
        sys.exit(f"step failed with exit status {r.returncode}: stopping")
    return r.stdout


if args.child:
    child(args.child)
else:
    import re
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    me = [sys.executable, os.path.join("tools", "hybrid_time.py"), "--iters", str(args.iters)]
    counts = {}
    with open(os.path.join(ROOT, "profiles", "hybrid_time.txt"), "w") as log:
        for shape in SHAPES:
            text = step(me + ["--child", shape], log)
            counts[shape] = (int(re.search(r"rows the gather reads\): (\d+)", text).group(1)),
                             int(re.search(r"rerank of the batch's (\d+) BM25 hits", text).group(1)))
    # a trace run of its own per shape: the per-kernel split, appended to the timing file
    with open(os.path.join(ROOT, "profiles", "hybrid_kernel_stats.txt"), "w") as table:
        for shape in SHAPES:
            out = os.path.join(ROOT, "build", "hybrid_rocprof_" + shape)
            os.makedirs(out, exist_ok=True)
            with open(os.path.join(ROOT, "build", f"hybrid_rocprof_{shape}.log"), "w") as log:
                step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"] + me +
                     ["--child", shape], log)
            stats = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))
            if not stats:
                sys.exit(f"no kernel statistics from the {shape} trace run: stopping")
            table.write(f"# rocprofv3 --kernel-trace --stats, {shape} shape: kernels of the library, all calls of the run\n")
            table.writelines(l for i, l in enumerate(open(stats[-1])) if i == 0 or "slg::" in l)
            with open(os.path.join(ROOT, "profiles", "hybrid_time.txt"), "a") as log:
                log.write(kernel_split(shape, stats[-1], *counts[shape]))
    print(open(os.path.join(ROOT, "profiles", "hybrid_time.txt")).read())
