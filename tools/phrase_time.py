"""Device time of a phrase-query batch (slg_batch_prepare_phrase -> slg_batch_run) after warm-up, on config 2's
corpus: 1M docs, 1024 three-term queries, k = 11, with synthetic positions (tf positions per posting: a start of
0 .. 15 taken from the posting's index, then steps of 3).

Without --child this is the driver: every GPU step is a child process under its own `timeout`, and the first
failure stops the run.  Steps: (1) the timing child: events around slg_batch_run of (a) the bool batch with one
MUST term group made from a scored term, (b) the same batch with that term as a one-term MUST phrase — which
adds the position lookup to the same search — and (c) the three scored terms as one three-term MUST phrase at
slop 0 and at slop 2; (2) one rocprofv3 --kernel-trace --stats run of the child, a run of its own without counters,
whose per-kernel table gives phrase_filter_kernel's own time beside bool_filter_kernel, score and select.
Output: profiles/phrase_time.txt.
usage (GPU box): python tools/phrase_time.py [--iters N] [--step-timeout S]"""
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

MUST = 0


def child():
    import numpy as np
    import torch
    from searchlite_amd import corpus, searcher
    n, vocab, nq, k = 1_000_000, 1 << 18, 1024, 11
    seg = corpus.zipf_segment(n, vocab, seed=42, n_threads=16)
    offs, terms, w = corpus.zipf_queries(nq, 3, rank_lo=64, rank_hi=8192, seed=7, vocab=vocab)
    st = np.asarray(terms, np.uint32).reshape(nq, 3)
    # synthetic positions: posting i has tf positions (i % 16) + 3 * j
    tfs = np.asarray(seg.tfs, np.int64)
    pos_offsets = np.concatenate([[0], np.cumsum(tfs)]).astype(np.uint64)
    first = np.repeat(pos_offsets[:-1].astype(np.int64), tfs)
    j = np.arange(int(pos_offsets[-1]), dtype=np.int64) - first
    positions = (np.repeat(np.arange(len(tfs), dtype=np.int64) % 16, tfs) + 3 * j).astype(np.uint32)
    per_q = (np.arange(nq + 1)).astype(np.uint32)
    term_group = dict(c_offsets=per_q, c_terms=st[:, :1].copy(), c_group=np.zeros(nq, np.uint32), g_offsets=per_q,
                      g_kind=np.full(nq, MUST, np.int32), q_min_should=0)

    def phrase(cols, slop):
        m = len(cols)
        return dict(p_offsets=per_q, p_kind=np.full(nq, MUST, np.int32), p_slop=np.full(nq, slop, np.uint32),
                    v_offsets=per_q, t_offsets=(np.arange(nq + 1) * m).astype(np.uint32),
                    t_terms=st[:, cols].reshape(-1, 1).copy())

    with searcher.GpuIndex([seg]) as ix:
        ix.set_stream(torch.cuda.current_stream().cuda_stream)
        ix.set_positions(0, pos_offsets, positions)
        batches = [("(1) bool batch, one MUST term group", ix.prepare(offs, terms, w, k, clauses=term_group)),
                   ("(2) the term as a one-term MUST phrase", ix.prepare(offs, terms, w, k, phrases=phrase([0], 0))),
                   ("(3a) three-term MUST phrase, slop 0", ix.prepare(offs, terms, w, k, phrases=phrase([0, 1, 2], 0))),
                   ("(3b) three-term MUST phrase, slop 2", ix.prepare(offs, terms, w, k, phrases=phrase([0, 1, 2], 2)))]

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

        ms = [timed(b.run) for _, b in batches]
        ms2 = [timed(b.run) for _, b in batches]
        accepted = [sum(int(s.scored_docs) for s in b.fetch(want_stats=True)[4]) for _, b in batches]
        n_slices = batches[0][1].info()["n_slices"]
        for _, b in batches:
            b.close()
    mean = [0.5 * (a + b) for a, b in zip(ms, ms2)]
    print(f"1M docs, {nq} three-term queries (term ranks 64..8192), k {k}; {int(pos_offsets[-1])} positions over "
          f"{len(tfs)} postings (tf per posting: mean {tfs.mean():.2f}, max {int(tfs.max())}); {n_slices} slices")
    for (name, _), a, b, acc in zip(batches, ms, ms2, accepted):
        print(f"  {name:42s} {a:8.3f} ms per batch (again after: {b:.3f}); accepted docs {acc}")
    print(f"  (2) / (1) = {mean[1] / mean[0]:.2f}, (3a) / (2) = {mean[2] / mean[1]:.2f}, (3b) / (2) = {mean[3] / mean[1]:.2f}",
          flush=True)


def kernel_split(csv_path):
    """per launch, from rocprofv3's kernel statistics (Name, Calls, TotalDurationNs)"""
    import csv
    stat = {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(csv_path))}
    out = ["per launch, from rocprofv3 --kernel-trace --stats (mean over the calls of the run; phrase_filter_kernel: "
           "over the three phrase batches):"]
    for key in ("score_uniform4_kernel", "select_topk_kernel", "merge_topk_kernel", "bool_filter_kernel", "phrase_filter_kernel"):
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
    me = [sys.executable, os.path.join("tools", "phrase_time.py"), "--iters", str(args.iters)]
    path = os.path.join(ROOT, "profiles", "phrase_time.txt")
    with open(path, "w") as log:
        step(me + ["--child"], log)
    out = os.path.join(ROOT, "build", "phrase_rocprof")  # a trace run of its own: the per-kernel split
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(ROOT, "build", "phrase_rocprof.log"), "w") as log:
        step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"] + me + ["--child"], log)
    stats = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))
    if not stats:
        sys.exit("no kernel statistics from the trace run: stopping")
    with open(path, "a") as log:
        log.write(kernel_split(stats[-1]))
    print(open(path).read())
