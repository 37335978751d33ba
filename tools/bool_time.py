"""Device time of a boolean-query batch (slg_batch_prepare_bool -> slg_batch_run) after warm-up, on config 2's
corpus: 1M docs, 1024 three-term queries, k = 11.

Without --child this is the driver: every GPU step is a child process under its own `timeout`, and the first
failure stops the run.  Steps: (1) the timing child: events around slg_batch_run of (a) the plain top-k batch,
(b) the same queries as a bool batch with an empty clause table — the cost of candidates mode alone — and (c) the
bool batch with, per query, one MUST term made from a scored term, one rare and one dense MUST_NOT term and the
three scored terms as SHOULD groups with min_should 2; (2) one rocprofv3 --kernel-trace --stats run of the child,
a run of its own without counters, whose per-kernel table gives bool_filter_kernel's own time beside score and
select.  Output: profiles/bool_time.txt.
usage (GPU box): python tools/bool_time.py [--iters N] [--step-timeout S]"""
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

MUST, SHOULD, MUST_NOT = 0, 1, 2


def child():
    import numpy as np
    import torch
    from searchlite_amd import corpus, searcher
    n, vocab, nq, k = 1_000_000, 1 << 18, 1024, 11
    seg = corpus.zipf_segment(n, vocab, seed=42, n_threads=16)
    offs, terms, w = corpus.zipf_queries(nq, 3, rank_lo=64, rank_hi=8192, seed=7, vocab=vocab)
    rare = corpus.zipf_queries(nq, 1, rank_lo=100000, rank_hi=200000, seed=9, vocab=vocab)[1].reshape(-1)
    dense = corpus.zipf_queries(nq, 1, rank_lo=8, rank_hi=64, seed=10, vocab=vocab)[1].reshape(-1)
    st = np.asarray(terms, np.uint32).reshape(nq, 3)
    # per query: MUST {scored 0}, MUST_NOT {rare}, MUST_NOT {dense}, SHOULD {scored 0}, {scored 1}, {scored 2}
    c_terms = np.stack([st[:, 0], rare, dense, st[:, 0], st[:, 1], st[:, 2]], axis=1).astype(np.uint32)
    full = dict(c_offsets=(np.arange(nq + 1) * 6).astype(np.uint32), c_terms=c_terms.reshape(-1, 1),
                c_group=np.tile(np.arange(6, dtype=np.uint32), nq), g_offsets=(np.arange(nq + 1) * 6).astype(np.uint32),
                g_kind=np.tile(np.array([MUST, MUST_NOT, MUST_NOT, SHOULD, SHOULD, SHOULD], np.int32), nq),
                q_min_should=2)
    zeros = np.zeros(nq + 1, np.uint32)
    empty = dict(c_offsets=zeros, c_terms=np.zeros((0, 1), np.uint32), c_group=np.zeros(0, np.uint32), g_offsets=zeros,
                 g_kind=np.zeros(0, np.int32))
    tid = c_terms.astype(np.int64).reshape(-1)
    df = (np.asarray(seg.term_offsets[tid + 1], np.int64) - np.asarray(seg.term_offsets[tid], np.int64))
    with searcher.GpuIndex([seg]) as ix:
        ix.set_stream(torch.cuda.current_stream().cuda_stream)
        plain = ix.prepare(offs, terms, w, k)
        cand = ix.prepare(offs, terms, w, k, clauses=empty)
        b = ix.prepare(offs, terms, w, k, clauses=full)

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
        bool_ms = timed(b.run)
        plain_ms2 = timed(plain.run)
        cand_ms2 = timed(cand.run)
        candidates = sum(int(s.scored_docs) for s in cand.fetch(want_stats=True)[4])
        got = b.fetch(want_stats=True)
        accepted = sum(int(s.scored_docs) for s in got[4])
        n_slices = b.info()["n_slices"]
        for x in (plain, cand, b):
            x.close()
    live = df > 0
    steps = np.ceil(np.log2(np.maximum(df[live], 1))) + 1
    per_q = live.reshape(nq, 6).sum(axis=1).mean()
    plain_m, cand_m = 0.5 * (plain_ms + plain_ms2), 0.5 * (cand_ms + cand_ms2)
    print(f"1M docs, {nq} three-term queries (term ranks 64..8192), k {k}; clause table per query: MUST {{scored 0}}, "
          f"MUST_NOT {{rare, ranks 100000..200000}}, MUST_NOT {{dense, ranks 8..64}}, SHOULD x 3 {{scored}}, min_should 2")
    print(f"  clause lists: df min {int(df.min())}, median {int(np.median(df))}, max {int(df.max())}; clause terms with "
          f"df > 0 per query: mean {per_q:.2f}; dependent loads per lookup (ceil(log2 df) + 1): mean {steps.mean():.1f}, "
          f"max {int(steps.max())}")
    print(f"  candidates per batch: {candidates} in {n_slices} slices; accepted: {accepted}; lookups if no lane left "
          f"early (candidates x clause terms with df > 0): {int(candidates * per_q)}")
    print(f"  (1) plain top-k batch (slg_batch_run):                  {plain_ms:8.3f} ms per batch (again after: {plain_ms2:.3f})")
    print(f"  (2) bool batch, empty clause table (candidates mode):   {cand_ms:8.3f} ms per batch (again after: {cand_ms2:.3f})")
    print(f"  (3) bool batch with the clause table:                   {bool_ms:8.3f} ms per batch")
    print(f"  (3) / (2) = {bool_ms / cand_m:.2f}, (2) / (1) = {cand_m / plain_m:.2f}; bool_filter_kernel by the difference of "
          f"the events: {bool_ms - cand_m:.3f} ms per batch", flush=True)


def kernel_split(csv_path):
    """per launch, from rocprofv3's kernel statistics (Name, Calls, TotalDurationNs)"""
    import csv
    stat = {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(csv_path))}
    out = ["per launch, from rocprofv3 --kernel-trace --stats (mean over the calls of the run):"]
    for key in ("score_uniform4_kernel", "select_topk_kernel", "merge_topk_kernel", "bool_filter_kernel"):
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
    me = [sys.executable, os.path.join("tools", "bool_time.py"), "--iters", str(args.iters)]
    path = os.path.join(ROOT, "profiles", "bool_time.txt")
    with open(path, "w") as log:
        step(me + ["--child"], log)
    out = os.path.join(ROOT, "build", "bool_rocprof")  # a trace run of its own: the per-kernel split
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(ROOT, "build", "bool_rocprof.log"), "w") as log:
        step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"] + me + ["--child"], log)
    stats = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))
    if not stats:
        sys.exit("no kernel statistics from the trace run: stopping")
    with open(path, "a") as log:
        log.write(kernel_split(stats[-1]))
    print(open(path).read())
