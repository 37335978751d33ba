"""Device time of explain (slg_batch_explain behind slg_batch_run) after warm-up, on config 5's text corpus: 1M
docs, 1024 three-term queries.  Three requests, and the rescore kernel beside them:
  rows10     rows 10 at k = 11, a plain batch
  rows1000   rows 1000 at k = 1001, a plain batch
  fscore8    rows 1000 at k = 1001, a function_score batch with 8 functions (weights, field_value_factor with sqrt
             and none, linear decay: the lean instantiation) over two columns
  rescore    k = 1001, window 1000, the rescore query = the first-pass query: rescore_kernel looks the same rows up
             in the same lists as explain does for rows1000 (the shape of profiles/rescore_time.txt), re-measured here

Without --child this is the driver: every GPU step is a child process under its own `timeout`, and the first
failure stops the run.  Steps: (1) the timing child per request: hip events around slg_batch_run alone and around
run + explain (which returns when the host arrays are filled: the copies are inside) in the same process, per
iteration, median and range; (2) per request one rocprofv3 --kernel-trace --stats run of the child, a run of its own
(the program after `--`), whose per-kernel table gives the explain kernel's own time.  Output:
profiles/explain_time.txt.
usage (GPU box): python tools/explain_time.py [--iters N] [--step-timeout S]"""
import argparse
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--child", default=None, help="rows10 | rows1000 | fscore8 | rescore (internal)")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--step-timeout", type=int, default=300)
args = ap.parse_args()

REQUESTS = ("rows10", "rows1000", "fscore8", "rescore")


def child(request):
    import numpy as np
    import torch
    from searchlite_amd import corpus, searcher
    n, vocab, nq = 1_000_000, 1 << 18, 1024
    k, rows = (11, 10) if request == "rows10" else (1001, 1000)
    seg = corpus.zipf_segment(n, vocab, seed=42, n_threads=16)
    offs, terms, w = corpus.zipf_queries(nq, 3, rank_lo=64, rank_hi=8192, seed=7, vocab=vocab)
    tid = np.asarray(terms, np.int64).reshape(-1)
    df = (np.asarray(seg.term_offsets[tid + 1], np.int64) - np.asarray(seg.term_offsets[tid], np.int64))
    with searcher.GpuIndex([seg]) as ix:
        ix.set_stream(torch.cuda.current_stream().cuda_stream)
        kinds = {}
        if request == "fscore8":
            rng = np.random.default_rng(3)
            one = np.arange(n + 1, dtype=np.uint32)
            pop = ix.add_agg_field([(one, rng.uniform(0.1, 1000.0, n))], np.float64)
            age = ix.add_agg_field([(one, rng.integers(0, 5001, n).astype(np.int64))], np.int64)
            fns = [dict(kind="weight", weight=1.5), dict(kind="field_value_factor", field=pop, modifier="sqrt"),
                   dict(kind="weight", weight=0.5), dict(kind="field_value_factor", field=age, factor=0.001),
                   dict(kind="decay", field=age, origin=2500.0, scale=3000.0, decay=0.5, function="linear"),
                   dict(kind="weight", weight=2.0), dict(kind="field_value_factor", field=pop, modifier="reciprocal"),
                   dict(kind="decay", field=pop, origin=500.0, scale=400.0, decay=0.25, function="linear")]
            kinds["fscore"] = [dict(functions=fns, score_mode="sum", boost_mode="sum")] * nq
        if request == "rescore":
            kinds["rescore"] = dict(q_offsets=offs, q_terms=terms, q_weights=w, window=1000, mode=0)
        b = ix.prepare(offs, terms, w, k, **kinds)

        def timed(f):
            f()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.iters):
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                e.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(e))
            return float(np.median(ms)), min(ms), max(ms)

        def run_and_explain():
            b.run()
            b.explain(rows)

        run_ms = timed(b.run)
        print(f"{request}: 1M docs, {nq} three-term queries (term ranks 64..8192), k {k}" +
              ("" if request == "rescore" else f", rows {rows}") + f", {args.iters} iterations after a warm-up")
        steps = np.ceil(np.log2(np.maximum(df, 1))) + 2
        print(f"  lists: df min {int(df.min())}, median {int(np.median(df))}, max {int(df.max())}; dependent loads per lookup "
              f"(ceil(log2 df) + 2): mean {steps.mean():.1f}, max {int(steps.max())}")
        print(f"  slg_batch_run alone:            median {run_ms[0]:8.3f} ms (min {run_ms[1]:.3f}, max {run_ms[2]:.3f})")
        if request != "rescore":
            both = timed(run_and_explain)
            run2 = timed(b.run)
            count = b.fetch()[3]
            ex = b.explain(rows)
            n_rows = int(np.minimum(count, rows).sum())
            print(f"  slg_batch_run + explain:        median {both[0]:8.3f} ms (min {both[1]:.3f}, max {both[2]:.3f})")
            print(f"  slg_batch_run alone, again:     median {run2[0]:8.3f} ms")
            print(f"  explain (upload, zero-fill, kernel, copies to the host arrays), by the difference: "
                  f"{both[0] - 0.5 * (run_ms[0] + run2[0]):8.3f} ms")
            print(f"  rows explained: {n_rows}, lookups: {3 * n_rows}, entries: {int(ex['n_functions'].sum())}, bytes to the "
                  f"host: {sum(a.nbytes for a in ex.values())}", flush=True)
        b.close()


def kernel_split(request, csv_path):
    """per launch, from rocprofv3's kernel statistics (Name, Calls, TotalDurationNs)"""
    import csv
    stat = {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(csv_path))}
    out = [f"{request}, per launch, from rocprofv3 --kernel-trace --stats (mean over the calls of the run):"]
    for key in ("score_uniform4_kernel", "fscore_kernel", "select_topk_kernel", "merge_topk_kernel", "rescore_kernel",
                "explain_kernel"):
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
    me = [sys.executable, os.path.join("tools", "explain_time.py"), "--iters", str(args.iters)]
    path = os.path.join(ROOT, "profiles", "explain_time.txt")
    with open(path, "w") as log:
        for request in REQUESTS:
            step(me + ["--child", request], log)
    for request in REQUESTS:  # a trace run of its own per request: the per-kernel split, appended to the timing file
        out = os.path.join(ROOT, "build", "explain_rocprof_" + request)
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(ROOT, "build", f"explain_rocprof_{request}.log"), "w") as log:
            step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"] + me +
                 ["--child", request], log)
        stats = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))
        if not stats:
            sys.exit(f"no kernel statistics from the {request} trace run: stopping")
        with open(path, "a") as log:
            log.write(kernel_split(request, stats[-1]))
    print(open(path).read())
