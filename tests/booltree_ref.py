"""Numpy model of the nested boolean matcher (slg_batch_prepare_bool_tree) over the oracle, on bool_ref's pattern.

  1. matches(): a direct recursive restatement of QueryEvaluator::matches_node (api/reader.rs:1485-1565) over the
     NESTED description of searchlite_amd/booltree.py — written from the reference, independent of
     compile_matchers: Bool walks must, must_not, its filter list and should with the default
     minimum_should_match rule (:1553-1561); DisMax is any-of and false when empty; QueryString is false without a
     group, rejects on a not-group, and counts its term groups against minimum_should_match.unwrap_or(1).
  2. compiled_masks(): the mask evaluator over the COMPILED arrays (the spec): leaves as bits 0-31, nodes as bits
     32-63, each node `every MUST && no MUST_NOT && popcount(SHOULD) >= min_should` in table order.
  3. reference(): oracle.search_batch_filtered with the accept mask as the query's filter (AND-ed with the query's
     own filter), and scored_docs(): the docs of the scored lists the matcher accepts.

filters: {filter id: [pass mask per segment, or None = the filter has no bitmap there and passes every doc]}."""
import numpy as np

from tests.bool_ref import NO_TERM, postings

MUST, SHOULD, MUST_NOT = 0, 1, 2


def group_holds(seg, s, terms):
    """term_group_matches (:1571-1580): a doc is held if any of the group's terms has a posting of it"""
    held = np.zeros(seg.n_docs, bool)
    for t in terms:
        tid = int(t) if np.ndim(t) == 0 else int(t[s])
        if tid != NO_TERM:
            held[postings(seg, tid)] = True
    return held


def matches(d, seg, s, filters=None):
    """matches_node over description d -> bool mask over the docs of segment s"""
    n = seg.n_docs
    if d == "match_all" or (isinstance(d, dict) and "match_all" in d):
        return np.ones(n, bool)
    (kind, body), = d.items()
    if kind == "term":
        return group_holds(seg, s, body)
    if kind == "query_string":
        terms, nots = list(body.get("terms", ())), list(body.get("not", ()))
        if not terms and not nots:
            return np.zeros(n, bool)
        ok = np.ones(n, bool)
        for g in nots:
            ok &= ~group_holds(seg, s, g)
        if not terms:
            return ok  # (not-groups only: true where none of them holds)
        cnt = np.zeros(n, np.int64)
        for g in terms:
            cnt += group_holds(seg, s, g)
        msm = body.get("minimum_should_match")
        return ok & (cnt >= (1 if msm is None else msm))
    if kind == "dis_max":
        out = np.zeros(n, bool)  # (empty: false)
        for c in body:
            out |= matches(c, seg, s, filters)
        return out
    if kind == "bool":
        must, should = list(body.get("must", ())), list(body.get("should", ()))
        must_not, flt = list(body.get("must_not", ())), list(body.get("filter", ()))
        ok = np.ones(n, bool)
        for c in must:
            ok &= matches(c, seg, s, filters)
        for c in must_not:
            ok &= ~matches(c, seg, s, filters)
        for f in flt:
            m = filters[f][s]
            if m is not None:
                ok &= np.asarray(m, bool)
        cnt = np.zeros(n, np.int64)
        for c in should:
            cnt += matches(c, seg, s, filters)
        msm = body.get("minimum_should_match")
        if msm is None:
            msm = 0 if not should else (1 if not must and not flt else 0)
        return ok & (cnt >= msm)
    raise ValueError(f"unknown matcher {d!r}")


def nested_masks(segs, queries, filters=None):
    """-> per query None (no matcher) or [mask per segment], by the recursive form"""
    return [None if d is None else [matches(d, seg, s, filters) for s, seg in enumerate(segs)] for d in queries]


def popcount64(x):
    x = np.asarray(x, np.uint64)
    out = np.zeros(x.shape, np.int64)
    for i in range(64):
        out += ((x >> np.uint64(i)) & np.uint64(1)).astype(np.int64)
    return out


def compiled_nodes(tree, q):
    """the node table of query q of a compiled spec as [(must, must_not, should, min_should)] over the 64 value bits"""
    nl = int(tree["g_offsets"][q + 1] - tree["g_offsets"][q]) + int(tree["f_offsets"][q + 1] - tree["f_offsets"][q])
    out = []
    for n in range(int(tree["n_offsets"][q]), int(tree["n_offsets"][q + 1])):
        m = [0, 0, 0]
        for e in range(int(tree["e_offsets"][n]), int(tree["e_offsets"][n + 1])):
            c, kind = int(tree["e_child"][e]), int(tree["e_kind"][e])
            m[kind] |= 1 << (c if c < nl else 32 + c - nl)
        out.append((m[MUST], m[MUST_NOT], m[SHOULD], int(tree["n_min_should"][n])))
    return out


def compiled_masks(segs, tree, filters=None):
    """-> per query None (no node) or [mask per segment], by the mask form over the compiled arrays"""
    nq = len(tree["n_offsets"]) - 1
    terms = np.asarray(tree["c_terms"], np.uint32).reshape(-1, len(segs))
    out = []
    for q in range(nq):
        nodes = compiled_nodes(tree, q)
        if not nodes:
            out.append(None)
            continue
        ng = int(tree["g_offsets"][q + 1] - tree["g_offsets"][q])
        per_seg = []
        for s, seg in enumerate(segs):
            val = np.zeros(seg.n_docs, np.uint64)
            for i in range(int(tree["c_offsets"][q]), int(tree["c_offsets"][q + 1])):
                t = int(terms[i, s])
                if t != NO_TERM:
                    val[postings(seg, t)] |= np.uint64(1 << int(tree["c_group"][i]))
            for j, f in enumerate(range(int(tree["f_offsets"][q]), int(tree["f_offsets"][q + 1]))):
                m = filters[int(tree["f_filter"][f])][s]
                passes = np.ones(seg.n_docs, bool) if m is None else np.asarray(m, bool)
                val[passes] |= np.uint64(1 << (ng + j))
            for i, (must, must_not, should, ms) in enumerate(nodes):
                v = ((val & np.uint64(must)) == np.uint64(must)) & ((val & np.uint64(must_not)) == np.uint64(0)) & \
                    (popcount64(val & np.uint64(should)) >= ms)
                val[v] |= np.uint64(1 << (32 + i))
            per_seg.append((val >> np.uint64(31 + len(nodes))) & np.uint64(1) != 0)
        out.append(per_seg)
    return out


def accept_masks(segs, queries, q_filter=None, filters=None):
    """the matcher masks (recursive form) AND-ed with each query's own filter -> per query [mask or None per segment]"""
    out = []
    for q, cm in enumerate(nested_masks(segs, queries, filters)):
        per_seg = [None] * len(segs) if cm is None else list(cm)
        f = int(q_filter[q]) if q_filter is not None else -1
        if f >= 0:
            per_seg = [fm if pm is None else (pm if fm is None else (pm & np.asarray(fm, bool)))
                       for pm, fm in zip(per_seg, filters[f])]
        out.append(per_seg)
    return out


def reference(oracle, segs, q_offsets, q_terms, q_weights, k, queries, q_filter=None, filters=None, strategy=None,
              **plans):
    """(doc, seg, score, count) of the tree batch whose matchers are the nested descriptions `queries`"""
    masks = accept_masks(segs, queries, q_filter, filters)
    nq = len(q_offsets) - 1
    return oracle.search_batch_filtered(segs, q_offsets, q_terms, q_weights, k, np.arange(nq), masks,
                                        strategy=oracle.BM25 if strategy is None else strategy, **plans)


def scored_docs(segs, q_offsets, q_terms, queries, filters=None):
    """per query: docs that hold a scored term and pass the matcher (no tombstone, no q_filter: slg_stats)"""
    terms = np.asarray(q_terms, np.uint32).reshape(-1, len(segs))
    masks = nested_masks(segs, queries, filters)
    out = np.zeros(len(q_offsets) - 1, np.uint64)
    for q in range(len(out)):
        for s, seg in enumerate(segs):
            hit = np.zeros(seg.n_docs, bool)
            for i in range(int(q_offsets[q]), int(q_offsets[q + 1])):
                if int(terms[i, s]) != NO_TERM:
                    hit[postings(seg, int(terms[i, s]))] = True
            if masks[q] is not None:
                hit &= masks[q][s]
            out[q] += int(hit.sum())
    return out


def random_tree(rng, vocab, depth, budget, filter_ids=()):
    """a random nested description of at most `depth` levels; budget: {"leaves": n, "nodes": n} left, counted
    as compile_matchers counts them (a term group or a filter id is a leaf, every other description a node)"""
    def term():
        budget["leaves"] -= 1
        return {"term": [int(x) for x in rng.choice(vocab, size=int(rng.integers(1, 3)), replace=False)]}

    def child(level):
        if level >= depth or budget["nodes"] <= 0 or rng.random() < 0.45:
            return term() if budget["leaves"] > 0 else "match_all_leafless"
        return node(level)

    def children(level, lo, hi):
        out = []
        for _ in range(int(rng.integers(lo, hi + 1))):
            if budget["leaves"] <= 0:
                break
            out.append(child(level))
        return [c for c in out if c != "match_all_leafless"]

    def node(level):
        budget["nodes"] -= 1
        kind = rng.choice(["bool", "bool", "dis_max", "query_string", "match_all"])
        if kind == "match_all":
            return "match_all"
        if kind == "dis_max":
            return {"dis_max": children(level + 1, 0, 3)}
        if kind == "query_string":
            body = {}
            for key in ("terms", "not"):
                n = int(rng.integers(0, 3))
                n = min(n, max(budget["leaves"], 0))
                budget["leaves"] -= n
                if n or rng.random() < 0.5:
                    body[key] = [[int(x) for x in rng.choice(vocab, size=int(rng.integers(1, 3)), replace=False)]
                                 for _ in range(n)]
            if rng.random() < 0.4:
                body["minimum_should_match"] = int(rng.integers(0, 3))
            return {"query_string": body}
        body = {}
        for key, hi in (("must", 2), ("should", 3), ("must_not", 2)):
            if rng.random() < 0.6:
                body[key] = children(level + 1, 0, hi)
        if filter_ids and budget["leaves"] > 0 and rng.random() < 0.3:
            budget["leaves"] -= 1
            body["filter"] = [int(rng.choice(filter_ids))]
        if rng.random() < 0.4:
            body["minimum_should_match"] = int(rng.integers(0, 4))
        return {"bool": body}

    return node(1)
