"""Device time of scan batches (slg_batch_prepare_scan -> slg_batch_run) after warm-up, on config 2's corpus: 1M docs
in one segment, 1024 queries.

Without --child this is the driver: every GPU step is a child process under its own `timeout`, and the first
failure stops the run.  Steps: (1) the timing child: events around slg_batch_run of
  (a) match_all, k = 11, score order — the truncated form: 11 candidates per slice, the rest counted;
  (b) constant_score over a range filter that passes about 10 % of the docs, one i64 sort ascending, k = 11;
  (c) match_all, k = 0, terms(8 keys) -> stats;
  (d) rank_feature log1p over an f64 column, k = 11;
(2) shape (b) again with the libraries built at other slice sizes (libsearchlite_gpu_scan<D>.so, built beforehand
with build.build_gpu(defines=["SLG_SCAN_SLICE_DOCS=<D>"], tag="scan<D>"); a missing one is skipped and said so);
(3) one rocprofv3 --kernel-trace --stats run of shape (b), a run of its own without counters, whose per-kernel table
gives scan_kernel's own time beside the select; the bytes it writes (8 per passing doc) and that figure as a share
of 8 TB/s follow from it.  No thresholds: the numbers are what they are.  Output: profiles/scan_time.txt.
usage (GPU box): python tools/scan_time.py [--iters N] [--step-timeout S] [--slice-docs 4096,65536]"""
import argparse
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--child", default="", help="(internal) the shapes to run, e.g. abcd")
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--slice-docs", default="4096,65536")
args = ap.parse_args()


def child(shapes):
    import numpy as np
    import torch
    from searchlite_amd import aggs as AG, corpus, searcher
    n, vocab, nq = 1_000_000, 1 << 18, 1024
    seg = corpus.zipf_segment(n, vocab, seed=42, n_threads=16)
    rng = np.random.default_rng(3)
    price = rng.integers(0, 1000, n).astype(np.int64)   # the range filter's and the sort's column
    pop = rng.uniform(0.0, 1000.0, n)                  # f64, one value per doc (stored without offsets)
    cat = rng.integers(0, 8, n).astype(np.uint32)
    csr = lambda v: (np.arange(n + 1, dtype=np.uint32), v)
    with searcher.GpuIndex([seg]) as ix:
        ix.set_stream(torch.cuda.current_stream().cuda_stream)
        flt = ix.add_filter_range([price], 0, 99)
        srt = ix.add_sort_field([csr(price)], np.int64)
        f_pop = ix.add_agg_field([csr(pop)], np.float64)
        f_cat = ix.add_agg_keyword_field([csr(cat)], 8)
        passing = int((price <= 99).sum())
        plan = AG.agg_spec({"c": {"type": "terms", "field": "cat", "aggs": {"s": {"type": "stats", "field": "pop"}}}},
                           {"cat": {"id": f_cat, "keys": [f"k{i}" for i in range(8)]}, "pop": {"id": f_pop}})
        made = {
            "a": ("match_all, k 11, score order (truncated)", lambda: ix.prepare_scan([{"match_all": {}}] * nq, 11)),
            "b": (f"constant_score over a range filter ({100.0 * passing / n:.1f} % pass), i64 sort asc, k 11",
                  lambda: ix.prepare_scan([{"constant_score": {"filter": flt, "boost": 2.0}}] * nq, 11, sort=[(srt, "asc")])),
            "c": ("match_all, k 0, terms(8) -> stats", lambda: ix.prepare_scan([{"match_all": {}}] * nq, 0, aggs=plan)),
            "d": ("rank_feature log1p (f64 column), k 11",
                  lambda: ix.prepare_scan([{"rank_feature": {"field": f_pop, "modifier": "log1p"}}] * nq, 11)),
        }

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

        print(f"1M docs in one segment, {nq} queries, {args.iters} runs after one warm-up; library {os.environ.get('SLG_LIB_TAG', 'product')}")
        for s in shapes:
            what, make = made[s]
            b = make()
            ms = timed(b.run)
            info, matched = b.info(), b.matched_counts()
            b.close()
            print(f"  ({s}) {what}:\n      {ms:9.3f} ms per batch; {info['n_slices']} slices of {info['scan_slice_docs']} docs, "
                  f"kernel {info['scan_kernel']}, matched per query {int(matched[0])}", flush=True)
        if "b" in shapes:
            print(f"  scan_kernel of (b) writes 8 B x {passing} passing docs x {nq} queries = {8 * passing * nq / 1e6:.1f} MB per batch",
                  flush=True)


def kernel_split(csv_path, written):
    """per launch, from rocprofv3's kernel statistics (Name, Calls, TotalDurationNs)"""
    import csv
    stat = {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(csv_path))}
    out = ["shape (b) per launch, from rocprofv3 --kernel-trace --stats (mean over the calls of the run):"]
    for key in ("scan_kernel", "select_sorted_kernel", "select_topk_kernel", "agg_kernel"):
        for name, (c, t) in stat.items():
            if key in name:
                ms = t / max(c, 1) / 1e6
                out.append(f"  {name[:70]:70s} {ms:8.3f} ms  ({c} calls)")
                if key == "scan_kernel" and written:
                    tbs = written / (ms * 1e-3) / 1e12
                    out.append(f"    its stores: {written / 1e6:.1f} MB per launch = {tbs:.3f} TB/s = {100.0 * tbs / 8.0:.1f} % of 8 TB/s "
                               f"(it also reads one bitmap word per 32 docs and query)")
    return "\n".join(out) + "\n"


def step(cmd, log, env=None):
    print("+", " ".join(cmd), flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(args.step_timeout)] + cmd, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, env=env)
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
    me = [sys.executable, os.path.join("tools", "scan_time.py"), "--iters", str(args.iters)]
    path = os.path.join(ROOT, "profiles", "scan_time.txt")
    with open(path, "w") as log:
        first = step(me + ["--child", "abcd"], log)
        for d in [x for x in args.slice_docs.split(",") if x]:
            lib = os.path.join(ROOT, "searchlite_amd", "lib", f"libsearchlite_gpu_scan{d}.so")
            if not os.path.exists(lib):
                log.write(f"(no library built at {d} docs per slice: skipped)\n")
                continue
            step(me + ["--child", "b"], log, env=dict(os.environ, SLG_LIB_TAG=f"scan{d}"))
    import re
    written = [8 * int(m.group(1)) * int(m.group(2)) for m in re.finditer(r"writes 8 B x (\d+) passing docs x (\d+) queries", first)]
    out = os.path.join(ROOT, "build", "scan_rocprof")  # a trace run of its own: the per-kernel split
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(ROOT, "build", "scan_rocprof.log"), "w") as log:
        step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"] + me + ["--child", "b"], log)
    stats = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))
    if not stats:
        sys.exit("no kernel statistics from the trace run: stopping")
    with open(path, "a") as log:
        log.write(kernel_split(stats[-1], written[0] if written else 0))
    print(open(path).read())
