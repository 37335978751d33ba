"""Device time of compound requests (slg_batch_prepare_request -> slg_batch_run) after warm-up, on config 2's corpus:
1M docs, 1024 three-term queries, k = 11.

Without --child this is the driver: the GPU step is a child process under its own `timeout`, and a failure stops the
run.  The child times four batches with events around slg_batch_run: (a) the bool batch of tools/bool_time.py (per
query one MUST term made from a scored term, one rare and one dense MUST_NOT term and the three scored terms as SHOULD
groups with min_should 2); (b) the same queries as an aggregation batch, terms over a keyword column of 8 keys ->
stats over an f64 column; (c) the compound bool + aggs batch; (d) bool + function_score (a weight under a function
filter and a linear decay, min_score) + a two-part sort + aggs + collapse over a keyword column of 64 keys with three
inner hits.  The only derivable expectation is (c) ~ (a) + (b)'s agg_kernel over fewer candidates; the figures are a
record, not a pass criterion.  Output: profiles/request_time.txt.
usage (GPU box): python tools/request_time.py [--iters N] [--step-timeout S]"""
import argparse
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
    from searchlite_amd import aggs as A, corpus, searcher
    n, vocab, nq, k = 1_000_000, 1 << 18, 1024, 11
    seg = corpus.zipf_segment(n, vocab, seed=42, n_threads=16)
    offs, terms, w = corpus.zipf_queries(nq, 3, rank_lo=64, rank_hi=8192, seed=7, vocab=vocab)
    rare = corpus.zipf_queries(nq, 1, rank_lo=100000, rank_hi=200000, seed=9, vocab=vocab)[1].reshape(-1)
    dense = corpus.zipf_queries(nq, 1, rank_lo=8, rank_hi=64, seed=10, vocab=vocab)[1].reshape(-1)
    st = np.asarray(terms, np.uint32).reshape(nq, 3)
    c_terms = np.stack([st[:, 0], rare, dense, st[:, 0], st[:, 1], st[:, 2]], axis=1).astype(np.uint32)
    clauses = dict(c_offsets=(np.arange(nq + 1) * 6).astype(np.uint32), c_terms=c_terms.reshape(-1, 1),
                   c_group=np.tile(np.arange(6, dtype=np.uint32), nq), g_offsets=(np.arange(nq + 1) * 6).astype(np.uint32),
                   g_kind=np.tile(np.array([MUST, MUST_NOT, MUST_NOT, SHOULD, SHOULD, SHOULD], np.int32), nq),
                   q_min_should=2)
    rng = np.random.default_rng(11)
    one = np.arange(n + 1, dtype=np.uint32)  # one value per doc
    with searcher.GpuIndex([seg]) as ix:
        ix.set_stream(torch.cuda.current_stream().cuda_stream)
        keys8 = [f"k{i}" for i in range(8)]
        fields = {"tag": {"id": ix.add_agg_keyword_field([(one, rng.integers(0, 8, n).astype(np.uint32))], 8), "keys": keys8},
                  "x": {"id": ix.add_agg_field([(one, rng.integers(-4096, 4096, n).astype(np.float64) / 64.0)], np.float64)},
                  "age": {"id": ix.add_agg_field([(one, rng.integers(0, 1000, n).astype(np.int64))], np.int64)}}
        grp = ix.add_agg_keyword_field([(one, rng.integers(0, 64, n).astype(np.uint32))], 64)
        low = ix.add_sort_field([(one, rng.integers(0, 8, n).astype(np.int64))], np.int64)
        half = ix.add_filter([rng.random(n) < 0.5])
        plan = A.agg_spec({"t": {"type": "terms", "field": "tag", "aggs": {"s": {"type": "stats", "field": "x"}}}}, fields)
        fs = [dict(functions=[dict(kind="weight", weight=1.5, filter=half),
                              dict(kind="decay", field=fields["age"]["id"], origin=500.0, scale=400.0, decay=0.5,
                                   function="linear")],
                   score_mode="sum", boost_mode="replace", min_score=1.0)] * nq
        sort = [(low, "asc"), ("_score", "desc")]
        collapse = dict(field=grp, group_limit=10, inner_size=3)
        batches = {
            "a": ("bool (slg_batch_prepare_bool)", ix.prepare(offs, terms, w, k, clauses=clauses)),
            "b": ("aggs, terms(8) -> stats (slg_batch_prepare_aggs)", ix.prepare(offs, terms, w, k, aggs=plan)),
            "c": ("bool + aggs (slg_batch_prepare_request)", ix.prepare_request(offs, terms, w, k, clauses=clauses, aggs=plan)),
            "d": ("bool + fscore + sort + aggs + collapse (slg_batch_prepare_request)",
                  ix.prepare_request(offs, terms, w, k, clauses=clauses, fscore=fs, sort=sort, aggs=plan, collapse=collapse)),
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

        ms = {name: timed(b.run) for name, (_, b) in batches.items()}
        again = {name: timed(b.run) for name, (_, b) in batches.items()}
        scored = {name: sum(int(s.scored_docs) for s in b.fetch(want_stats=True)[4]) for name, (_, b) in batches.items()}
        matched = {name: int(b.matched_counts().sum()) for name, (_, b) in batches.items() if name != "a"}
        for _, b in batches.values():
            b.close()
    print(f"1M docs, {nq} three-term queries (term ranks 64..8192), k {k}, {args.iters} runs after one warm-up run; events "
          f"around slg_batch_run")
    for name, (what, _) in batches.items():
        print(f"  ({name}) {what:68s} {ms[name]:8.3f} ms per batch (again after: {again[name]:.3f}); scored_docs "
              f"{scored[name]}" + (f", matched {matched[name]}" if name in matched else ""))
    mean = {name: 0.5 * (ms[name] + again[name]) for name in ms}
    print(f"  (c) - (a) = {mean['c'] - mean['a']:.3f} ms: the collectors over the clause stage's survivors; (b) - plain "
          f"scoring is not split here (tools/agg_time.py); (c) / ((a) + (b)) = {mean['c'] / (mean['a'] + mean['b']):.2f}; "
          f"(d) / (c) = {mean['d'] / mean['c']:.2f}", flush=True)


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
    path = os.path.join(ROOT, "profiles", "request_time.txt")
    with open(path, "w") as log:
        step([sys.executable, os.path.join("tools", "request_time.py"), "--iters", str(args.iters), "--child"], log)
    print(open(path).read())
