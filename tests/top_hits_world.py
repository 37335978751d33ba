"""The worlds of tests/test_gpu_top_hits.py, built without a device so that tests/test_top_hits_world.py can check on
the CPU, with tests/top_hits_ref.py alone, that they give what the GPU cases need.

build(): two segments of 1500 / 1100 docs over a vocabulary of 40 (the second with tombstones) and 12 queries:
  0        the three most frequent terms: nearly every live doc
  1 .. 7   three random terms
  8        one crafted list in each segment, 100 + 60 docs: more than a wave, fewer than four waves' worth
  9        a crafted list of 40 docs of segment 0: fewer than a wave
  10       no term
  11       one doc
Sort fields (name -> (values[seg][doc], is_float), as tests/collapse_ref.py reads them): `low` an i64 of 8 values on
every doc (long ties), `f64` 0 .. 2 values out of a pool with NaN, -0.0 and infinities (a doc without one is Missing),
`tie` the same value on every doc (every key equal: segment, then doc), `n` an i64 of many values.
Aggregation columns (field -> values[seg][doc], as tests/agg_ref.py reads them):
  tag    keyword, 6 keys: no value (the `missing` row), one, two different, or the same key twice
  len    keyword laid over query 0's matched docs so that its keys have exactly LENGTHS docs there
  x      f64 multiples of 0.25 in [-6, 6], 0 .. 2 values
  ts     i64 milliseconds over 40 days, 0 .. 2 values
  wide   i64 in [0, 9000), one value: a histogram of interval 1 has 9000 rows (its counts beyond the LDS home of the
         aggregation kernel, its cursors beyond the LDS of the top_hits kernel), of interval 2 4500 (counts in LDS,
         cursors not), of interval 100 90 (both in LDS)
and the doc masks `half` (a filter aggregation) and `third` (a query's doc filter).

build_many(): six segments of 50 docs and two queries, so that a query has more slices than the workgroup has waves.
"""
import numpy as np

from tests import collapse_world as CW
from tests.util import _append_lists, random_queries, random_segment

NO_TERM = 0xFFFFFFFF
SIZES = (1500, 1100)
VOCAB = 40
KEYS = [f"k{i}" for i in range(6)]
LENGTHS = (0, 1, 63, 64, 65, 128, 129)  # around the 64-at-a-time read of a run
LEN_KEYS = [f"n{n}" for n in LENGTHS]
KEYS_OF = {"tag": KEYS, "len": LEN_KEYS}
DAY = 86_400_000
WIDE = 9000


def hits_of(all_hits):
    doc, seg, score, count = all_hits
    return [[(int(seg[q, i]), int(doc[q, i]), score[q, i]) for i in range(int(count[q]))] for q in range(len(count))]


def build(oracle):
    rng = np.random.default_rng(20261020)
    segs = [random_segment(rng, n, VOCAB, 25, k1=0.9, b=0.4) for n in SIZES]
    pick = lambda n, m: np.sort(rng.choice(n, size=m, replace=False))
    # segment 0: term 40 in one doc, 41 in 40 docs, 42 in 100 docs; segment 1: term 40 in 60 docs
    segs[0] = _append_lists(segs[0], [([17], [2]), (pick(SIZES[0], 40), np.ones(40)), (pick(SIZES[0], 100), np.ones(100))])
    segs[1] = _append_lists(segs[1], [(pick(SIZES[1], 60), np.ones(60))])
    segs[1] = CW.tombstoned(segs[1], rng, 0.15)
    offs, terms, w = random_queries(rng, 12, 3, VOCAB, n_segs=2, weights=True)
    terms[0:3, :] = np.array([0, 1, 2], np.uint32)[:, None]
    for q in (8, 9, 10, 11):
        terms[3 * q:3 * q + 3, :] = NO_TERM
    terms[3 * 8, :] = [42, 40]
    terms[3 * 9, 0] = 41
    terms[3 * 11, 0] = 40
    n_docs = [s.n_docs for s in segs]
    k_all = sum(n_docs)
    all_hits = oracle.search_batch(segs, offs, terms, w, k_all, strategy=oracle.BM25)
    hits = hits_of(all_hits)

    fields = CW.make_fields(rng, n_docs)
    fields["tie"] = ([[[5]] * n for n in n_docs], False)
    fields["n"] = ([[[int(rng.integers(0, 10000))] for _ in range(n)] for n in n_docs], False)

    def tag():
        r = rng.random()
        a, b = (KEYS[int(j)] for j in rng.integers(0, len(KEYS), 2))
        return [] if r < 0.1 else [a] if r < 0.7 else [a, a] if r < 0.8 or a == b else [a, b]
    cols = {"tag": [[tag() for _ in range(n)] for n in n_docs]}
    # `len`: query 0's matched docs in a shuffled order take the keys, LENGTHS[i] docs each; nobody else has a value
    cols["len"] = [[[] for _ in range(n)] for n in n_docs]
    order = [hits[0][i] for i in rng.permutation(len(hits[0]))]
    at = 0
    for key, n in zip(LEN_KEYS, LENGTHS):
        for seg, doc, _ in order[at:at + n]:
            cols["len"][seg][doc] = [key]
        at += n
    cols["x"] = [[[float(v) / 4.0 for v in rng.integers(-24, 25, int(rng.integers(0, 3)))] for _ in range(n)] for n in n_docs]
    cols["ts"] = [[[int(rng.integers(0, 40)) * DAY + int(rng.integers(0, DAY)) for _ in range(int(rng.integers(0, 3)))]
                   for _ in range(n)] for n in n_docs]
    cols["wide"] = [[[int(rng.integers(0, WIDE))] for _ in range(n)] for n in n_docs]
    for s in range(2):  # the ends of the range exist, so the table has exactly WIDE rows
        cols["wide"][s][0], cols["wide"][s][1] = [0], [WIDE - 1]
    masks = {"half": [rng.random(n) < 0.5 for n in n_docs], "third": [rng.random(n) < 0.33 for n in n_docs]}
    return dict(segs=segs, offs=offs, terms=terms, w=w, n_docs=n_docs, k_all=k_all, all=all_hits, hits=hits,
                fields=fields, cols=cols, masks=masks)


def build_many(oracle):
    rng = np.random.default_rng(20261021)
    segs = [random_segment(rng, 50, 10, 12, k1=0.9, b=0.4) for _ in range(6)]
    offs, terms, w = random_queries(rng, 2, 3, 10, n_segs=6, weights=True)
    terms[0:3, :] = np.array([0, 1, 2], np.uint32)[:, None]
    n_docs = [s.n_docs for s in segs]
    all_hits = oracle.search_batch(segs, offs, terms, w, sum(n_docs), strategy=oracle.BM25)
    fields = {"low": ([[[int(rng.integers(0, 8))] for _ in range(n)] for n in n_docs], False)}
    return dict(segs=segs, offs=offs, terms=terms, w=w, n_docs=n_docs, k_all=sum(n_docs), all=all_hits,
                hits=hits_of(all_hits), fields=fields, cols={}, masks={})


def ref_nodes(request, plan, layout):
    """the top_hits nodes of `request` as tests/top_hits_ref.expected takes them, in the order of plan.top_hits_nodes
    (searchlite_amd.aggs.agg_spec); layout: agg_date_ref.ref_layout(plan.nodes, ...)"""
    out = []
    for th in plan.top_hits_nodes:
        parent = None if th["parent"] < 0 else plan.nodes[th["parent"]]["body"]
        body = request[th["name"]] if parent is None else parent["aggs"][th["name"]]
        sort = [(p["field"], p.get("order") or ("desc" if p["field"] == "_score" else "asc")) for p in body.get("sort") or []]
        out.append({"parent": parent, "parent_lay": None if parent is None else layout[th["parent"]],
                    "from": th["from"], "size": th["size"], "sort": sort})
    return out
