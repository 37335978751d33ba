"""Device time of the query rescore (slg_batch_prepare_rescore -> slg_batch_run) after warm-up, on config 5's
text corpus: 1M docs, 1024 three-term queries, k = 1001, window 1000, three rescore terms per query, drawn from
the dense and from the selective term rank range of tools/hybrid_time.py.

Without --child this is the driver: every GPU step is a child process under its own `timeout`, and the first
failure stops the run.  Steps: (1) the timing child per shape: events around slg_batch_run of the rescore batch
and of the same batch without rescore (score + select), measured in the same run; their difference is the
rescore kernel; (2) per shape one rocprofv3 --kernel-trace --stats run of the child, a run of its own, whose
per-kernel table gives the rescore kernel's own time beside score and select.  Output: profiles/rescore_time.txt.
usage (GPU box): python tools/rescore_time.py [--iters N] [--step-timeout S]"""
import argparse
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--child", default=None, help="dense | selective (internal)")
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--step-timeout", type=int, default=300)
args = ap.parse_args()

SHAPES = {"dense": (64, 8192), "selective": (60000, 200000)}  # term rank ranges of the rescore terms


def child(shape):
    import numpy as np
    import torch
    from searchlite_amd import corpus, searcher
    n, vocab, nq, k, window = 1_000_000, 1 << 18, 1024, 1001, 1000
    seg = corpus.zipf_segment(n, vocab, seed=42, n_threads=16)
    offs, terms, w = corpus.zipf_queries(nq, 3, rank_lo=64, rank_hi=8192, seed=7, vocab=vocab)
    lo, hi = SHAPES[shape]
    ro, rt, rw = corpus.zipf_queries(nq, 3, rank_lo=lo, rank_hi=hi, seed=8, vocab=vocab)
    rescore = dict(q_offsets=ro, q_terms=rt, q_weights=rw, window=window, mode=0)
    tid = np.asarray(rt, np.int64).reshape(-1)
    df = (np.asarray(seg.term_offsets[tid + 1], np.int64) - np.asarray(seg.term_offsets[tid], np.int64))
    with searcher.GpuIndex([seg]) as ix:
        ix.set_stream(torch.cuda.current_stream().cuda_stream)
        plain = ix.prepare(offs, terms, w, k)
        b = ix.prepare(offs, terms, w, k, rescore=rescore)

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

        plain_ms = timed(plain.run)
        both_ms = timed(b.run)
        plain_ms2 = timed(plain.run)
        count = b.fetch()[3]
        flag = b.rescore_details()[2]
        rows = int(np.minimum(count, window).sum())
        plain.close()
        b.close()
    steps = np.ceil(np.log2(np.maximum(df, 1))) + 2
    print(f"{shape}: 1M docs, {nq} three-term queries (term ranks 64..8192), k {k}, window {window}, three rescore "
          f"terms per query (term ranks {lo}..{hi})")
    print(f"  rescore lists: df min {int(df.min())}, median {int(np.median(df))}, max {int(df.max())}; dependent loads "
          f"per lookup (ceil(log2 df) + 2): mean {steps.mean():.1f}, max {int(steps.max())}")
    print(f"  window rows: {rows}, lookups: {3 * rows}, rows rescored: {int(flag.sum())}")
    print(f"  score + select (slg_batch_run without rescore): {plain_ms:8.3f} ms per batch (again after: {plain_ms2:.3f})")
    print(f"  score + select + rescore (slg_batch_run):       {both_ms:8.3f} ms per batch")
    print(f"  rescore kernel, by the difference of the events: {both_ms - 0.5 * (plain_ms + plain_ms2):8.3f} ms per batch",
          flush=True)


def kernel_split(shape, csv_path):
    """per launch, from rocprofv3's kernel statistics (Name, Calls, TotalDurationNs)"""
    import csv
    stat = {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(csv_path))}
    out = [f"{shape} shape, per launch, from rocprofv3 --kernel-trace --stats (mean over the calls of the run):"]
    for key in ("score_uniform4_kernel", "select_topk_kernel", "merge_topk_kernel", "rescore_kernel"):
        for name, (c, t) in stat.items():
            if key in name:
                out.append(f"  {name[:70]:70s} {t / max(c, 1) / 1e6:8.3f} ms  ({c} calls)")
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
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    me = [sys.executable, os.path.join("tools", "rescore_time.py"), "--iters", str(args.iters)]
    path = os.path.join(ROOT, "profiles", "rescore_time.txt")
    with open(path, "w") as log:
        for shape in SHAPES:
            step(me + ["--child", shape], log)
    for shape in SHAPES:  # a trace run of its own per shape: the per-kernel split, appended to the timing file
        out = os.path.join(ROOT, "build", "rescore_rocprof_" + shape)
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(ROOT, "build", f"rescore_rocprof_{shape}.log"), "w") as log:
            step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"] + me +
                 ["--child", shape], log)
        stats = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))
        if not stats:
            sys.exit(f"no kernel statistics from the {shape} trace run: stopping")
        with open(path, "a") as log:
            log.write(kernel_split(shape, stats[-1]))
    print(open(path).read())
