#!/usr/bin/env python3
"""Generates tests/golden/recipes_sort.npz: the `total_time_minutes` fast field (examples/recipes/schema.json:
i64, fast) of the reference's example corpus, in the doc order of recipes.npz (recipes.json "ext_ids"), as a
CSR of values per doc (one value each in this corpus).  Data, not source: it lets tests/test_gpu_sort.py sort
the recipes corpus by `total_time_minutes asc` (recipes/queries/collapse-quick-by-cuisine.json) on a machine
without the reference.  Run where the reference's examples/ directory is mounted:
    python tests/golden/make_sort_golden.py <path to examples/recipes/data.jsonl>"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main(data_jsonl):
    ext_ids = json.load(open(os.path.join(HERE, "recipes.json")))["ext_ids"]
    by_id = {}
    with open(data_jsonl) as f:
        for line in f:
            doc = json.loads(line)
            by_id[doc["doc_id"]] = doc
    offs, vals = [0], []
    for eid in ext_ids:
        v = by_id[eid].get("total_time_minutes")
        vs = [] if v is None else (v if isinstance(v, list) else [v])
        vals += [int(x) for x in vs]
        offs.append(len(vals))
    np.savez_compressed(os.path.join(HERE, "recipes_sort.npz"),
                        total_time_minutes_offsets=np.array(offs, dtype=np.uint32),
                        total_time_minutes=np.array(vals, dtype=np.int64))
    print("recipes_sort:", len(ext_ids), "docs,", len(set(vals)), "distinct total_time_minutes")


if __name__ == "__main__":
    main(sys.argv[1])
