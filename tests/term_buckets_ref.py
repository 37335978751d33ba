"""significant_terms and rare_terms restated (SignificantTermsCollector, compute_background_counts, RareTermsCollector,
the merge and finalize: query/aggs/mod.rs:131-359, 2110-2181, 2395-2424, 2515-2595).

A world is: cols[field][seg][doc] = the doc's keyword values (a list of strings), n_docs[seg], deleted[seg] = a set of
doc ids (or None), masks[name][seg][doc] = the doc passes the filter, and the collected docs of one query as (seg, doc)
pairs.  per_segment=True is the reference, literally: a collector per segment, finished (filtered by the count bound,
sorted, truncated to size), the intermediates merged in segment order (sorted and truncated again at every merge) and
finalized.  per_segment=False is the device's deliberate deviation: the counts of all segments are added up before
anything is filtered or truncated.  In BOTH modes a significant bucket's bg_count is the sum of the background counts of
the segments in whose foreground the key occurs, which is what the reference's merge adds up.

Keys order as Rust Strings do: by their UTF-8 bytes.  A bucket carries "docs", the (seg, doc) pairs counted in it, for
the children; strip() removes them.
"""
import struct

MAX_BUCKETS = 10_000


def key_order(k):
    return k.encode("utf-8")


def distinct(values):
    seen, out = set(), []
    for v in values:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def background(col_seg, n_docs, deleted, mask):
    """compute_background_counts of one segment: (counts by key, bg_total)"""
    counts, total = {}, 0
    for d in range(n_docs):
        if deleted is not None and d in deleted:
            continue
        if mask is not None and not mask[d]:
            continue
        total += 1
        for v in distinct(col_seg[d]):
            counts[v] = counts.get(v, 0) + 1
    return counts, total


def foreground(col_seg, docs):
    """the collect() of one collector: (docs by key in arrival order, docs with a value)"""
    buckets, doc_count = {}, 0
    for d in docs:
        values = col_seg[d]
        if not values:
            continue
        doc_count += 1
        for v in distinct(values):
            buckets.setdefault(v, []).append(d)
    return buckets, doc_count


def terms_cmp_key(b):
    return (-b["doc_count"], key_order(b["key"]))


def rare_cmp_key(b):
    return (b["doc_count"], key_order(b["key"]))


def limit_of(size, n):
    return min(n if size is None else size, MAX_BUCKETS)


def by_segment(hits, n_segs):
    out = [[] for _ in range(n_segs)]
    for seg, d in hits:
        out[seg].append((seg, d))
    return out


def score_of(doc_count_b, doc_count, bg_count_b, bg_count):
    if doc_count > 0 and bg_count > 0 and bg_count_b > 0:
        return (float(doc_count_b) / float(doc_count)) / (float(bg_count_b) / float(bg_count))
    return 0.0


def score_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def significant(body, cols, n_docs, deleted, masks, hits, per_segment):
    """-> {"type": "significant_terms", "buckets": [{"key", "doc_count", "bg_count", "score", "docs"}], "doc_count",
    "bg_count"}"""
    field, size = body["field"], body.get("size")
    mdc = body.get("min_doc_count")
    min_count = 1 if mdc is None else int(mdc)
    bf = body.get("background_filter")
    n_segs = len(n_docs)
    col = cols[field]
    segs = []  # per segment: (buckets {key: docs}, doc_count, bg counts, bg_total)
    for s, docs in enumerate(by_segment(hits, n_segs)):
        bg, total = background(col[s], n_docs[s], deleted[s] if deleted else None,
                               None if bf is None else masks[bf["name"]][s])
        fg, dc = foreground(col[s], [d for _, d in docs])
        segs.append(({k: [(s, d) for d in v] for k, v in fg.items()}, dc, bg, total))
    doc_count = sum(x[1] for x in segs)
    bg_count = sum(x[3] for x in segs)
    if per_segment:
        merged = None
        for fg, _, bg, _ in segs:
            fin = [{"key": k, "doc_count": len(v), "bg_count": bg.get(k, 0), "docs": list(v)} for k, v in fg.items()
                   if len(v) >= min_count]
            fin.sort(key=terms_cmp_key)
            fin = fin[:limit_of(size, len(fin))]
            if merged is None:
                merged = fin
                continue
            index = {b["key"]: b for b in merged}
            for b in fin:
                if b["key"] in index:
                    t = index[b["key"]]
                    t["doc_count"] += b["doc_count"]
                    t["bg_count"] += b["bg_count"]
                    t["docs"] += b["docs"]
                else:
                    index[b["key"]] = b
                    merged.append(b)
            merged.sort(key=terms_cmp_key)
            merged = merged[:limit_of(size, len(merged))]
        buckets = merged or []
    else:
        acc = {}
        for fg, _, bg, _ in segs:
            for k, v in fg.items():
                b = acc.setdefault(k, {"key": k, "doc_count": 0, "bg_count": 0, "docs": []})
                b["doc_count"] += len(v)
                b["bg_count"] += bg.get(k, 0)  # (this segment's foreground holds the key)
                b["docs"] += v
        buckets = [b for b in acc.values() if b["doc_count"] >= min_count]
        buckets.sort(key=terms_cmp_key)
        buckets = buckets[:limit_of(size, len(buckets))]
    for b in buckets:
        b["score"] = score_of(b["doc_count"], doc_count, b["bg_count"], bg_count)
    buckets.sort(key=lambda b: (-b["score"],) + terms_cmp_key(b))
    buckets = buckets[:limit_of(size, len(buckets))]
    return {"type": "significant_terms", "buckets": buckets, "doc_count": doc_count, "bg_count": bg_count}


def rare(body, cols, n_docs, hits, per_segment):
    """-> {"type": "rare_terms", "buckets": [{"key", "doc_count", "docs"}]}"""
    field, size = body["field"], body.get("size")
    mdc = body.get("max_doc_count")
    max_count = 1 if mdc is None else int(mdc)
    n_segs = len(n_docs)
    col = cols[field]
    keep = lambda bs: [b for b in bs if 0 < b["doc_count"] <= max_count]
    per = []
    for s, docs in enumerate(by_segment(hits, n_segs)):
        fg, _ = foreground(col[s], [d for _, d in docs])
        per.append([{"key": k, "doc_count": len(v), "docs": [(s, d) for d in v]} for k, v in fg.items()])
    if per_segment:
        merged = None
        for bs in per:
            fin = sorted(keep(bs), key=rare_cmp_key)
            fin = fin[:limit_of(size, len(fin))]
            if merged is None:
                merged = fin
                continue
            index = {b["key"]: b for b in merged}
            for b in fin:
                if b["key"] in index:
                    index[b["key"]]["doc_count"] += b["doc_count"]
                    index[b["key"]]["docs"] += b["docs"]
                else:
                    index[b["key"]] = b
                    merged.append(b)
            merged = sorted(keep(merged), key=rare_cmp_key)
            merged = merged[:limit_of(size, len(merged))]
        buckets = merged or []
    else:
        acc = {}
        for bs in per:
            for b in bs:
                t = acc.setdefault(b["key"], {"key": b["key"], "doc_count": 0, "docs": []})
                t["doc_count"] += b["doc_count"]
                t["docs"] += b["docs"]
        buckets = keep(acc.values())
    buckets = sorted(buckets, key=rare_cmp_key)
    buckets = buckets[:limit_of(size, len(buckets))]
    return {"type": "rare_terms", "buckets": buckets}


def respond(body, cols, n_docs, deleted, masks, hits, per_segment):
    if body["type"] == "significant_terms":
        return significant(body, cols, n_docs, deleted, masks, hits, per_segment)
    return rare(body, cols, n_docs, hits, per_segment)


def strip(resp):
    """the response without the buckets' doc lists"""
    out = dict(resp)
    out["buckets"] = [{k: v for k, v in b.items() if k != "docs"} for b in resp["buckets"]]
    return out
