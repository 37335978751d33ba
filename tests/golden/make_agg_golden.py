#!/usr/bin/env python3
"""Generates tests/golden/recipes_aggs.npz: the columns the aggregations of the reference's example request
recipes/queries/agg-macros-by-diet.json read, in the doc order of recipes.npz (recipes.json "ext_ids"):
  diet_offsets / diet_ords / diet_keys   the keyword field `dietary_tags` as a CSR of ordinals into the sorted
                                         list of its distinct values (examples/recipes/schema.json: keyword, fast)
  protein_offsets / protein              `nutrition.per_serving.protein_g` (f64) as a CSR of values per doc
(`total_time_minutes` is in recipes_sort.npz).  Data, not source: it lets tests/test_gpu_aggs.py aggregate the
recipes corpus on a machine without the reference.  Run where the reference's examples/ directory is mounted:
    python tests/golden/make_agg_golden.py <path to examples/recipes/data.jsonl>"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def values_at(doc, path):
    cur = [doc]
    for part in path.split("."):
        nxt = []
        for c in cur:
            if isinstance(c, dict) and part in c and c[part] is not None:
                v = c[part]
                nxt += v if isinstance(v, list) else [v]
        cur = nxt
    return cur


def main(data_jsonl):
    ext_ids = json.load(open(os.path.join(HERE, "recipes.json")))["ext_ids"]
    by_id = {}
    with open(data_jsonl) as f:
        for line in f:
            doc = json.loads(line)
            by_id[doc["doc_id"]] = doc
    tags = [[str(t) for t in values_at(by_id[e], "dietary_tags")] for e in ext_ids]
    keys = sorted({t for ts in tags for t in ts})
    ord_of = {k: i for i, k in enumerate(keys)}
    d_offs, d_ords, p_offs, p_vals = [0], [], [0], []
    for e, ts in zip(ext_ids, tags):
        d_ords += [ord_of[t] for t in ts]
        d_offs.append(len(d_ords))
        p_vals += [float(x) for x in values_at(by_id[e], "nutrition.per_serving.protein_g")]
        p_offs.append(len(p_vals))
    np.savez_compressed(os.path.join(HERE, "recipes_aggs.npz"),
                        diet_offsets=np.array(d_offs, dtype=np.uint32), diet_ords=np.array(d_ords, dtype=np.uint32),
                        diet_keys=np.array(keys, dtype=np.str_),
                        protein_offsets=np.array(p_offs, dtype=np.uint32), protein=np.array(p_vals, dtype=np.float64))
    print("recipes_aggs:", len(ext_ids), "docs,", len(keys), "dietary_tags keys,", len(d_ords), "tag values,",
          len(p_vals), "protein values")


if __name__ == "__main__":
    main(sys.argv[1])
