#!/usr/bin/env python3
"""Generates tests/golden/recipes_collapse.npz: the column the collapse of the reference's example request
recipes/queries/collapse-quick-by-cuisine.json groups by, in the doc order of recipes.npz (recipes.json "ext_ids"):
  cuisine_offsets / cuisine_ords / cuisine_keys   the keyword field `cuisine` as a CSR of ordinals into the sorted
                                                  list of its distinct values (examples/recipes/schema.json:
                                                  keyword, fast)
(`total_time_minutes`, the request's sort and inner sort, is in recipes_sort.npz).  Data, not source: it lets
tests/test_gpu_collapse.py collapse the recipes corpus on a machine without the reference.  Run where the
reference's examples/ directory is mounted:
    python tests/golden/make_collapse_golden.py <path to examples/recipes/data.jsonl>"""
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

    def values(doc):
        v = doc.get("cuisine")
        return [] if v is None else [str(x) for x in (v if isinstance(v, list) else [v])]
    per_doc = [values(by_id[e]) for e in ext_ids]
    keys = sorted({c for cs in per_doc for c in cs})
    ord_of = {k: i for i, k in enumerate(keys)}
    offs, ords = [0], []
    for cs in per_doc:
        ords += [ord_of[c] for c in cs]
        offs.append(len(ords))
    np.savez_compressed(os.path.join(HERE, "recipes_collapse.npz"),
                        cuisine_offsets=np.array(offs, dtype=np.uint32), cuisine_ords=np.array(ords, dtype=np.uint32),
                        cuisine_keys=np.array(keys, dtype=np.str_))
    print("recipes_collapse:", len(ext_ids), "docs,", len(keys), "cuisine keys,", len(ords), "values,",
          sum(len(cs) != 1 for cs in per_doc), "docs without exactly one")


if __name__ == "__main__":
    main(sys.argv[1])
