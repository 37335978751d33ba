"""What a nested filter costs to MAKE, two ways, on config 2's corpus: 1M docs, a nested path with about 2 objects per
doc (0-4), one keyword nested column of 20 keys and one i64 nested column, a value per object each.  The filter is
And(Nested(c, author = x), Nested(c, score >= y)): both must hold for ONE object.

  (a) today's route at the parent commit: the nested part evaluated with numpy on the host (vectorised over the
      objects, folded to docs through the prefix sums), registered through slg_index_add_filter, and named by a
      FILTER_ID leaf of a tree registered through slg_index_add_filter_trees;
  (b) slg_index_add_nested_filter_trees with 1 tree, and with 16 trees (16 different filters of that shape) in one
      call.

Both are host clocks around calls that end in a stream synchronise, mean of --iters runs after a warm-up; the
bitmaps of the two sides are compared for equality.  Without --child this is the driver: the GPU step is a child
process under its own `timeout`.  Output: profiles/nested_filter_time.txt.
usage (GPU box): python tools/nested_filter_time.py [--iters N] [--docs N] [--step-timeout S]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
    counts = rng.integers(0, 5, n).astype(np.uint32)
    base = np.zeros(n + 1, np.uint32)
    base[1:] = np.cumsum(counts)
    n_obj = int(base[-1])
    author = rng.integers(0, 20, n_obj).astype(np.uint32)
    score = rng.integers(0, 100, n_obj).astype(np.int64)
    return counts, base, author, score


def filter_of(j):
    """the j-th filter of the shape: (author key, lowest score)"""
    return j % 20, 40 + 3 * (j % 16)


def host_mask(base, author, score, j):
    """the nested part on the host: the objects that pass, folded to docs through the prefix sums"""
    import numpy as np
    key, lo = filter_of(j)
    hit = np.concatenate([[0], np.cumsum((author == key) & (score >= lo))])
    return hit[base[1:]] > hit[base[:-1]]


def tree_of(path, fields, j):
    key, lo = filter_of(j)
    nodes = [dict(kind=0, field=fields[0], ord_begin=0, n_ords_in=1), dict(kind=2, field=fields[1], lo_i=lo, hi_i=2**63 - 1),
             dict(kind=4, arity=2), dict(kind=7, field=0)]
    return [(path, 0, 3), (-1, 3, 1)], nodes, [key]


def child():
    import numpy as np
    n = args.docs
    counts, base, author, score = world(n)
    masks = [host_mask(base, author, score, j) for j in range(16)]
    print(f"{n} docs, {len(author)} objects of one nested path (0-4 per doc); author: 20 keys, score: i64, a value per object each")
    print(f"  filter 0 passes {int(masks[0].sum())} docs")
    if args.dry:
        return
    import torch  # noqa: F401  (the HIP runtime the library binds to)
    from searchlite_amd import corpus, searcher
    seg = corpus.zipf_segment(n, 1 << 18, seed=42, n_threads=16)
    one_each = np.arange(len(author) + 1, dtype=np.uint32)
    clock = time.perf_counter
    with searcher.GpuIndex([seg]) as ix:
        path = ix.add_nested_path([counts])
        fields = [ix.add_nested_keyword_field(path, [(base, one_each, author)], 20),
                  ix.add_nested_field(path, [(base, one_each, score)], np.int64)]

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

        def today(js):
            """numpy, add_filter, then a FILTER_ID tree per filter in one add_filter_trees call"""
            made = [ix.add_filter([host_mask(base, author, score, j)]) for j in js]
            return made + ix.add_filter_trees([([dict(kind=3, filter_id=f)], []) for f in made])

        t_eval = timed(lambda: [host_mask(base, author, score, 0)], lambda m: None)
        t_a1 = timed(lambda: today([0]), drop)
        t_a16 = timed(lambda: today(range(16)), drop)
        t_b1 = timed(lambda: ix.add_nested_filter_trees([tree_of(path, fields, 0)]), drop)
        t_b16 = timed(lambda: ix.add_nested_filter_trees([tree_of(path, fields, j) for j in range(16)]), drop)
        t_a1_again = timed(lambda: today([0]), drop)
        # the result is the same filter
        got = ix.add_nested_filter_trees([tree_of(path, fields, j) for j in range(16)])
        old = today(range(16))
        for j, f in enumerate(got):
            new_bits = ix.fetch_filter(f)[0]
            assert np.array_equal(new_bits, masks[j]) and np.array_equal(new_bits, ix.fetch_filter(old[16 + j])[0]), j
        drop(got + old)
    print(f"  (a) numpy + slg_index_add_filter + FILTER_ID tree, 1 filter: {t_a1:9.3f} ms (again after: {t_a1_again:.3f}); "
          f"the numpy evaluation alone {t_eval:.3f}")
    print(f"  (a) the same for 16 filters (16 masks, 1 tree call):         {t_a16:9.3f} ms")
    print(f"  (b) slg_index_add_nested_filter_trees, 1 tree:               {t_b1:9.3f} ms")
    print(f"  (b) slg_index_add_nested_filter_trees, 16 trees, 1 call:     {t_b16:9.3f} ms")
    print(f"  (b) / (a): 1 filter {t_b1 / t_a1:.4f}, 16 filters {t_b16 / t_a16:.4f}; the 16 bitmaps of (b) equal the numpy "
          f"masks and the bitmaps of (a)", flush=True)


if args.child:
    child()
else:
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    me = [sys.executable, os.path.join("tools", "nested_filter_time.py"), "--iters", str(args.iters), "--docs", str(args.docs)]
    path = os.path.join(ROOT, "profiles", "nested_filter_time.txt")
    print("+", " ".join(me + ["--child"]), flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(args.step_timeout)] + me + ["--child"], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        print(r.stdout[-2000:])
        sys.exit(f"step failed with exit status {r.returncode}: stopping")
    with open(path, "w") as log:
        log.write(r.stdout)
    print(r.stdout)
