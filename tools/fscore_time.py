"""Device time of a function_score batch (slg_batch_prepare_fscore -> slg_batch_run) after warm-up, on config 2's
corpus: 1M docs, 1024 three-term queries, k = 11.

Without --child this is the driver: every GPU step is a child process under its own `timeout`, and the first
failure stops the run.  Steps: (1) the timing child: events around slg_batch_run of (a) the plain top-k batch,
(b) the same queries as a function_score batch whose spec gives no query any work — the cost of candidates mode
alone — and (c) the batch with, per query, one field_value_factor log1p over a popularity column plus one decay
gauss over an age column, summed, with a min_score chosen on the host so that about half of the candidates drop;
(2) one rocprofv3 --kernel-trace --stats run of the child, a run of its own without counters, whose per-kernel
table gives fscore_kernel's own time beside score and select.  The ratios to read: (c) / (b), which is this kernel,
and (b) / (a), which is candidates mode and not this kernel's cost.  Output: profiles/fscore_time.txt.
usage (GPU box): python tools/fscore_time.py [--iters N] [--step-timeout S]"""
import argparse
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--child", action="store_true", help="(internal)")
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--step-timeout", type=int, default=300)
args = ap.parse_args()


def child():
    import numpy as np
    import torch
    from searchlite_amd import corpus, searcher
    n, vocab, nq, k = 1_000_000, 1 << 18, 1024, 11
    seg = corpus.zipf_segment(n, vocab, seed=42, n_threads=16)
    offs, terms, w = corpus.zipf_queries(nq, 3, rank_lo=64, rank_hi=8192, seed=7, vocab=vocab)
    rng = np.random.default_rng(3)
    pop = rng.uniform(0.0, 1000.0, n)             # f64, one value per doc (stored without offsets)
    age = rng.integers(0, 5000, n).astype(np.int64)
    csr = lambda v: (np.arange(n + 1, dtype=np.uint32), v)
    with searcher.GpuIndex([seg]) as ix:
        ix.set_stream(torch.cuda.current_stream().cuda_stream)
        f_pop, f_age = ix.add_agg_field([csr(pop)], np.float64), ix.add_agg_field([csr(age)], np.int64)
        fns = [dict(kind="field_value_factor", field=f_pop, modifier="log1p"),
               dict(kind="decay", field=f_age, origin=0.0, scale=2500.0, decay=0.5, function="gauss")]
        # the median of the two functions' sum over all docs: about half of any query's candidates lie below it
        value = np.log1p(pop).astype(np.float32) + np.power(0.5, (age / 2500.0) ** 2).astype(np.float32)
        min_score = float(np.median(value))
        spec = dict(functions=fns, score_mode="sum", boost_mode="replace", min_score=min_score)
        plain = ix.prepare(offs, terms, w, k)
        cand = ix.prepare(offs, terms, w, k, fscore=[None] * nq)
        b = ix.prepare(offs, terms, w, k, fscore=[spec] * nq)

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
        cand_ms = timed(cand.run)
        fs_ms = timed(b.run)
        plain_ms2 = timed(plain.run)
        cand_ms2 = timed(cand.run)
        candidates = sum(int(s.scored_docs) for s in cand.fetch(want_stats=True)[4])
        kept = sum(int(s.scored_docs) for s in b.fetch(want_stats=True)[4])
        info = b.info()
        for x in (plain, cand, b):
            x.close()
    plain_m, cand_m = 0.5 * (plain_ms + plain_ms2), 0.5 * (cand_ms + cand_ms2)
    print(f"1M docs, {nq} three-term queries (term ranks 64..8192), k {k}; per query: field_value_factor log1p (f64 column) + "
          f"decay gauss (i64 column), score_mode sum, boost_mode replace, min_score {min_score:.4f}")
    print(f"  candidates per batch: {candidates} in {info['n_slices']} slices; kept: {kept} "
          f"({100.0 * kept / max(candidates, 1):.1f} %); kernel: {info['fscore_kernel']}")
    print(f"  (1) plain top-k batch (slg_batch_run):                      {plain_ms:8.3f} ms per batch (again after: {plain_ms2:.3f})")
    print(f"  (2) function_score batch, no query has work (candidates):   {cand_ms:8.3f} ms per batch (again after: {cand_ms2:.3f})")
    print(f"  (3) function_score batch, log1p + gauss, min_score:         {fs_ms:8.3f} ms per batch")
    print(f"  (3) / (2) = {fs_ms / cand_m:.2f}, (2) / (1) = {cand_m / plain_m:.2f}; fscore_kernel by the difference of the "
          f"events: {fs_ms - cand_m:.3f} ms per batch (the select then ranks fewer candidates)", flush=True)


def kernel_split(csv_path):
    """per launch, from rocprofv3's kernel statistics (Name, Calls, TotalDurationNs)"""
    import csv
    stat = {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(csv_path))}
    out = ["per launch, from rocprofv3 --kernel-trace --stats (mean over the calls of the run):"]
    for key in ("score_uniform4_kernel", "select_topk_kernel", "merge_topk_kernel", "fscore_kernel"):
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
    child()
else:
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    me = [sys.executable, os.path.join("tools", "fscore_time.py"), "--iters", str(args.iters)]
    path = os.path.join(ROOT, "profiles", "fscore_time.txt")
    with open(path, "w") as log:
        step(me + ["--child"], log)
    out = os.path.join(ROOT, "build", "fscore_rocprof")  # a trace run of its own: the per-kernel split
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(ROOT, "build", "fscore_rocprof.log"), "w") as log:
        step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"] + me + ["--child"], log)
    stats = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))
    if not stats:
        sys.exit("no kernel statistics from the trace run: stopping")
    with open(path, "a") as log:
        log.write(kernel_split(stats[-1]))
    print(open(path).read())
