"""What a filter costs to MAKE, two ways, on config 2's corpus: 1M docs, one keyword column of 20 keys (one value per
doc), one multi-valued keyword column (0-3 of 50 keys per doc) and one i64 column.  The filter is
And(KeywordEq(cat), KeywordIn(tags, 3 keys), I64Range(year)).

  (a) the mask evaluated with numpy on the host, packed and registered through slg_index_add_filter: the only way
      before filter trees;
  (b) slg_index_add_filter_trees with 1 tree, and with 16 trees (16 different filters of that shape) in one call.

Both are host clocks around calls that end in a stream synchronise.  Without --child this is the driver: every GPU
step is a child process under its own `timeout`, and the first failure stops the run.  Steps: (1) the timing child;
(2) one rocprofv3 --kernel-trace --stats run of the child, a run of its own without counters, whose per-kernel table
gives filter_tree_kernel's own time; the bytes the kernel has to read (computed from the columns' shapes) over that
time are set against the 6.29 TB/s a float4 copy reaches on an MI355X.  Output: profiles/filter_tree_time.txt.
usage (GPU box): python tools/filter_tree_time.py [--iters N] [--docs N] [--step-timeout S]"""
import argparse
import glob
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.29e12  # bytes/s of a float4 copy on an MI355X (8.0 TB/s is the HBM3E figure)

ap = argparse.ArgumentParser()
ap.add_argument("--child", action="store_true", help="(internal)")
ap.add_argument("--dry", action="store_true", help="(internal) the host half only: no device is touched")
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--step-timeout", type=int, default=300)
args = ap.parse_args()


def world(n):
    import numpy as np
    rng = np.random.default_rng(5)
    cat = rng.integers(0, 20, n).astype(np.uint32)
    counts = rng.integers(0, 4, n)
    tag_offs = np.zeros(n + 1, np.uint32)
    tag_offs[1:] = np.cumsum(counts)
    tags = rng.integers(0, 50, int(tag_offs[-1])).astype(np.uint32)
    year = rng.integers(1990, 2026, n).astype(np.int64)
    return cat, tag_offs, tags, year


def filter_of(j):
    """the j-th filter of the shape: (cat key, tag keys, year range)"""
    return j % 20, [(3 * j) % 50, (3 * j + 1) % 50, (3 * j + 17) % 50], 2000 + j % 10, 2015 + j % 10


def host_mask(cat, tag_offs, tags, year, j):
    import numpy as np
    key, tag_keys, lo, hi = filter_of(j)
    hit = np.concatenate([[0], np.cumsum(np.isin(tags, tag_keys))])
    return (cat == key) & (hit[tag_offs[1:]] > hit[tag_offs[:-1]]) & (year >= lo) & (year <= hi)


def tree_of(ids, j):
    key, tag_keys, lo, hi = filter_of(j)
    nodes = [dict(kind=0, field=ids[0], ord_begin=0, n_ords_in=1), dict(kind=0, field=ids[1], ord_begin=1, n_ords_in=3),
             dict(kind=2, field=ids[2], lo_i=lo, hi_i=hi), dict(kind=4, arity=3)]
    return nodes, [key] + tag_keys


def child():
    import numpy as np
    n = args.docs
    cat, tag_offs, tags, year = world(n)
    masks = [host_mask(cat, tag_offs, tags, year, j) for j in range(16)]
    # what the kernel has to read for one tree (one value per doc without offsets: cat, year) and what it writes
    read_bytes = cat.nbytes + tag_offs.nbytes + tags.nbytes + year.nbytes
    write_bytes = (n + 31) // 32 * 4
    print(f"{n} docs; cat: 20 keys, one per doc; tags: 50 keys, {len(tags)} values in a CSR; year: i64, one per doc")
    print(f"  filter 0 passes {int(masks[0].sum())} docs; one tree reads at most {read_bytes} bytes "
          f"(a doc's tag walk stops at its first hit) and writes {write_bytes}")
    if args.dry:
        return
    import torch  # noqa: F401  (the HIP runtime the library binds to)
    from searchlite_amd import corpus, searcher
    seg = corpus.zipf_segment(n, 1 << 18, seed=42, n_threads=16)
    dense = lambda v: (np.arange(n + 1, dtype=np.uint32), v)
    clock = time.perf_counter
    with searcher.GpuIndex([seg]) as ix:
        ids = [ix.add_agg_keyword_field([dense(cat)], 20), ix.add_agg_keyword_field([(tag_offs, tags)], 50),
               ix.add_agg_field([dense(year)], np.int64)]

        def timed(f, undo):
            undo(f())  # warm-up
            total = 0.0
            for _ in range(args.iters):
                t0 = clock()
                out = f()
                total += clock() - t0
                undo(out)
            return 1e3 * total / args.iters

        drop = lambda fs: [ix.remove_filter(f) for f in fs]
        t_eval = timed(lambda: [host_mask(cat, tag_offs, tags, year, 0)], lambda m: None)
        t_reg = timed(lambda: [ix.add_filter([masks[0]])], drop)
        t_a1 = timed(lambda: [ix.add_filter([host_mask(cat, tag_offs, tags, year, 0)])], drop)
        t_a16 = timed(lambda: [ix.add_filter([host_mask(cat, tag_offs, tags, year, j)]) for j in range(16)], drop)
        t_b1 = timed(lambda: ix.add_filter_trees([tree_of(ids, 0)]), drop)
        t_b16 = timed(lambda: ix.add_filter_trees([tree_of(ids, j) for j in range(16)]), drop)
        t_a1_again = timed(lambda: [ix.add_filter([host_mask(cat, tag_offs, tags, year, 0)])], drop)
        # the result is the same filter
        got = ix.add_filter_trees([tree_of(ids, j) for j in range(16)])
        for j, f in enumerate(got):
            assert np.array_equal(ix.fetch_filter(f)[0], masks[j]), j
        drop(got)
    print(f"  (a) numpy mask + slg_index_add_filter, 1 filter:   {t_a1:9.3f} ms (again after: {t_a1_again:.3f}); the mask "
          f"alone {t_eval:.3f}, packing and registering a ready mask {t_reg:.3f}")
    print(f"  (a) the same for 16 filters, 16 calls:             {t_a16:9.3f} ms")
    print(f"  (b) slg_index_add_filter_trees, 1 tree:            {t_b1:9.3f} ms")
    print(f"  (b) slg_index_add_filter_trees, 16 trees, 1 call:  {t_b16:9.3f} ms")
    print(f"  (b) / (a): 1 filter {t_b1 / t_a1:.4f}, 16 filters {t_b16 / t_a16:.4f}; the 16 bitmaps equal the numpy masks", flush=True)
    print(f"KERNEL_BYTES {read_bytes} {write_bytes}")


def kernel_line(csv_path, text):
    """filter_tree_kernel per launch, from rocprofv3's kernel statistics (Name, Calls, TotalDurationNs): the child
    launches it 2 x (iters + 1) + 1 times, half of them with 1 tree and the rest with 16, so the mean is over both;
    the per-tree figure divides by the trees launched"""
    import csv
    read_bytes, write_bytes = [int(x) for x in text.split("KERNEL_BYTES")[1].split()[:2]]
    out = []
    for r in csv.DictReader(open(csv_path)):
        if "filter_tree_kernel" in r["Name"]:
            calls, total = int(r["Calls"]), float(r["TotalDurationNs"])
            trees = (args.iters + 1) * 17 + 16
            per_tree = total / trees
            out.append(f"filter_tree_kernel, from rocprofv3 --kernel-trace --stats: {calls} launches, {total / 1e6:.3f} ms in all, "
                       f"{trees} trees: {per_tree / 1e3:.1f} us per tree\n")
            out.append(f"  bytes read / time: {read_bytes / (per_tree * 1e-9) / 1e12:.2f} TB/s per tree against a copy rate of "
                       f"{COPY_RATE / 1e12:.2f} TB/s ({100.0 * read_bytes / (per_tree * 1e-9) / COPY_RATE:.0f} %; the 16 trees "
                       f"of one launch read the same columns, so the later ones find them in the caches)\n")
    return "".join(out) or "filter_tree_kernel is not in the kernel statistics\n"


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
    me = [sys.executable, os.path.join("tools", "filter_tree_time.py"), "--iters", str(args.iters), "--docs", str(args.docs)]
    path = os.path.join(ROOT, "profiles", "filter_tree_time.txt")
    with open(path, "w") as log:
        text = step(me + ["--child"], log)
    out = os.path.join(ROOT, "build", "filter_tree_rocprof")  # a trace run of its own: the kernel's time
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(ROOT, "build", "filter_tree_rocprof.log"), "w") as log:
        step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"] + me + ["--child"], log)
    stats = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))
    if not stats:
        sys.exit("no kernel statistics from the trace run: stopping")
    with open(path, "a") as log:
        log.write(kernel_line(stats[-1], text))
    print(open(path).read())
