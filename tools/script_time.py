"""Device time of a script_score batch (slg_batch_prepare_script -> slg_batch_run) after warm-up, on config 2's
corpus: 1M docs, 1024 three-term queries, k = 11.

Without --child this is the driver: every GPU step is a child process under its own `timeout`, and the first
failure stops the run.  Steps: (1) the timing child: events around slg_batch_run of (1) the plain top-k batch,
(2) the same queries as a script batch in which no query has a program — the cost of candidates mode alone —
(3) the batch with `_score * (1 + popularity / 10) + recency * w` per query (an f64 and an i64 column), and (4) the
batch with a 64-instruction program of depth 8 over the same columns; (2) one rocprofv3 --kernel-trace --stats run of
the child, a run of its own without counters, whose per-kernel table gives script_kernel's own time beside score and
select.  The ratios to read: (3) / (2) and (4) / (2), which are this kernel, and (2) / (1), which is candidates mode
and not this kernel's cost.  No threshold is set on any of them.  Output: profiles/script_time.txt.
usage (GPU box): python tools/script_time.py [--iters N] [--step-timeout S]"""
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


def deep_program(f_pop, f_rec):
    """64 instructions, depth 8: eight pushes, seven operators over them, 24 x (push, operator), a negation"""
    from searchlite_amd import _native as N
    push = [(N.SCRIPT_PUSH_SCORE, 0), (N.SCRIPT_PUSH_FIELD, f_pop), (N.SCRIPT_PUSH_CONST, 0.001), (N.SCRIPT_PUSH_FIELD, f_rec),
            (N.SCRIPT_PUSH_CONST, 1.5), (N.SCRIPT_PUSH_FIELD, f_pop), (N.SCRIPT_PUSH_CONST, 10.0), (N.SCRIPT_PUSH_FIELD, f_rec)]
    ops = [N.SCRIPT_ADD, N.SCRIPT_DIV, N.SCRIPT_SUB, N.SCRIPT_MUL, N.SCRIPT_ADD, N.SCRIPT_MUL, N.SCRIPT_ADD]
    prog = push + [(op, 0) for op in ops]
    for i in range(24):
        prog += [push[1 + i % 7], ((N.SCRIPT_ADD, N.SCRIPT_SUB, N.SCRIPT_MUL)[i % 3] if i % 8 else N.SCRIPT_DIV, 0)]
    return prog + [(N.SCRIPT_NEG, 0)]


def child():
    import numpy as np
    import torch
    from searchlite_amd import corpus, searcher
    from searchlite_amd.script import compile_script
    n, vocab, nq, k = 1_000_000, 1 << 18, 1024, 11
    seg = corpus.zipf_segment(n, vocab, seed=42, n_threads=16)
    offs, terms, w = corpus.zipf_queries(nq, 3, rank_lo=64, rank_hi=8192, seed=7, vocab=vocab)
    rng = np.random.default_rng(3)
    pop = rng.uniform(0.0, 1000.0, n)             # f64, one value per doc (stored without offsets)
    rec = rng.integers(1, 5000, n).astype(np.int64)
    csr = lambda v: (np.arange(n + 1, dtype=np.uint32), v)
    with searcher.GpuIndex([seg]) as ix:
        ix.set_stream(torch.cuda.current_stream().cuda_stream)
        f_pop, f_rec = ix.add_agg_field([csr(pop)], np.float64), ix.add_agg_field([csr(rec)], np.int64)
        text = "_score * (1 + popularity / 10) + recency * w"
        short = compile_script(text, dict(w=0.001), dict(popularity=f_pop, recency=f_rec))
        deep = deep_program(f_pop, f_rec)
        assert len(deep) == 64
        plain = ix.prepare(offs, terms, w, k)
        cand = ix.prepare(offs, terms, w, k, script=[None] * nq)
        b3 = ix.prepare(offs, terms, w, k, script=[short] * nq)
        b4 = ix.prepare(offs, terms, w, k, script=[deep] * nq)

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
        s3_ms = timed(b3.run)
        s4_ms = timed(b4.run)
        plain_ms2 = timed(plain.run)
        cand_ms2 = timed(cand.run)
        candidates = sum(int(s.scored_docs) for s in cand.fetch(want_stats=True)[4])
        kept3 = sum(int(s.scored_docs) for s in b3.fetch(want_stats=True)[4])
        kept4 = sum(int(s.scored_docs) for s in b4.fetch(want_stats=True)[4])
        info3, info4 = b3.info(), b4.info()
        for x in (plain, cand, b3, b4):
            x.close()
    plain_m, cand_m = 0.5 * (plain_ms + plain_ms2), 0.5 * (cand_ms + cand_ms2)
    print(f"1M docs, {nq} three-term queries (term ranks 64..8192), k {k}; columns: popularity f64, recency i64")
    print(f"  candidates per batch: {candidates} in {info3['n_slices']} slices; kept by (3): {kept3}, by (4): {kept4}")
    print(f"  (1) plain top-k batch (slg_batch_run):                         {plain_ms:8.3f} ms per batch (again after: {plain_ms2:.3f})")
    print(f"  (2) script batch, no query has a program (candidates):         {cand_ms:8.3f} ms per batch (again after: {cand_ms2:.3f})")
    print(f"  (3) `{text}`, {len(short)} instructions, depth {info3['script_max_depth']}:")
    print(f"                                                                 {s3_ms:8.3f} ms per batch")
    print(f"  (4) {len(deep)} instructions, depth {info4['script_max_depth']}:                               {s4_ms:8.3f} ms per batch")
    print(f"  (3) / (2) = {s3_ms / cand_m:.2f}, (4) / (2) = {s4_ms / cand_m:.2f}, (2) / (1) = {cand_m / plain_m:.2f}; script_kernel by "
          f"the difference of the events: (3) {s3_ms - cand_m:.3f} ms, (4) {s4_ms - cand_m:.3f} ms per batch", flush=True)


def kernel_split(csv_path):
    """per launch, from rocprofv3's kernel statistics (Name, Calls, TotalDurationNs)"""
    import csv
    stat = {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(csv_path))}
    out = ["per launch, from rocprofv3 --kernel-trace --stats (mean over the calls of the run; script_kernel: (3) and (4) together):"]
    for key in ("score_uniform4_kernel", "select_topk_kernel", "merge_topk_kernel", "script_kernel"):
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
    me = [sys.executable, os.path.join("tools", "script_time.py"), "--iters", str(args.iters)]
    path = os.path.join(ROOT, "profiles", "script_time.txt")
    with open(path, "w") as log:
        step(me + ["--child"], log)
    out = os.path.join(ROOT, "build", "script_rocprof")  # a trace run of its own: the per-kernel split
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(ROOT, "build", "script_rocprof.log"), "w") as log:
        step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"] + me + ["--child"], log)
    stats = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))
    if not stats:
        sys.exit("no kernel statistics from the trace run: stopping")
    with open(path, "a") as log:
        log.write(kernel_split(stats[-1]))
    print(open(path).read())
