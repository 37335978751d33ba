"""Nested boolean matchers for GpuIndex.search_batch_bool_tree: the reference's matcher tree
(QueryEvaluator::matches_node, api/reader.rs:1485-1565) folded into the one node form of slg_bool_tree_spec.

A matcher is described per query as

    {"bool": {"must": [...], "should": [...], "must_not": [...], "filter": [filter ids],
              "minimum_should_match": n}}                                  every key optional
    {"dis_max": [...]}
    {"query_string": {"terms": [[term, ...], ...], "not": [[term, ...], ...], "minimum_should_match": n}}
    {"term": [term, ...]}            one term group; a term is one id for every segment or one id per segment
    "match_all"
    None                             no matcher: the query is left as it is

where the children of bool and dis_max are such descriptions again.  compile_matchers() applies the folding rules
of include/searchlite_gpu.h: every node becomes a list of (child, kind) pairs plus a min_should, a Bool's filter
list becomes MUST filter leaves, a term group under a node is a leaf of that node, and a matcher that is one term
group gets one node with that leaf as its MUST child.  A phrase has no device form in a tree: SLG_ERR_UNSUPPORTED."""
import numpy as np

from . import _native as N

MUST, SHOULD, MUST_NOT = 0, 1, 2


class _Query:
    """the leaves and nodes of one query while its description is walked"""

    def __init__(self, n_segs):
        self.n_segs = n_segs
        self.groups = []   # term groups: [[ids per segment], ...]
        self.filters = []  # filter leaves: ids
        self.nodes = []    # (edges [(child, kind)], min_should); child = ("t", i) / ("f", i) / ("n", j)

    def term_group(self, terms):
        terms = list(terms)
        if not terms:
            raise N.SlgError(N.ERR_INVALID, "a term group without a term")
        self.groups.append([[int(t)] * self.n_segs if np.ndim(t) == 0 else [int(x) for x in t] for t in terms])
        return ("t", len(self.groups) - 1)

    def node(self, edges, min_should):
        self.nodes.append((edges, int(min_should)))
        return ("n", len(self.nodes) - 1)

    def walk(self, d):
        """-> the value of description d: a leaf or a node (children first: the table is in post-order)"""
        if isinstance(d, str):
            if d != "match_all":
                raise N.SlgError(N.ERR_INVALID, f"unknown matcher {d!r}")
            return self.node([], 0)
        if not isinstance(d, dict) or len(d) != 1:
            raise N.SlgError(N.ERR_INVALID, f"a matcher is a dict with one key, 'match_all' or None: {d!r}")
        (kind, body), = d.items()
        if kind == "term":
            return self.term_group(body)
        if kind == "phrase":
            raise N.SlgError(N.ERR_UNSUPPORTED, "a phrase leaf in a matcher tree is not built on the device")
        if kind == "match_all":
            return self.node([], 0)
        if kind == "dis_max":
            edges = [(self.walk(c), SHOULD) for c in body]
            return self.node(edges, 1)  # (empty: no children, min_should 1 — never true)
        if kind == "query_string":
            nots = [(self.term_group(g), MUST_NOT) for g in body.get("not", ())]
            terms = [(self.term_group(g), SHOULD) for g in body.get("terms", ())]
            if not nots and not terms:
                return self.node([], 1)  # never true
            msm = body.get("minimum_should_match")
            return self.node(nots + terms, (1 if msm is None else msm) if terms else 0)
        if kind == "bool":
            must = [(self.walk(c), MUST) for c in body.get("must", ())]
            must_not = [(self.walk(c), MUST_NOT) for c in body.get("must_not", ())]
            flt = []
            for f in body.get("filter", ()):
                self.filters.append(int(f))
                flt.append((("f", len(self.filters) - 1), MUST))
            should = [(self.walk(c), SHOULD) for c in body.get("should", ())]
            msm = body.get("minimum_should_match")
            if msm is None:
                msm = 0 if not should else (1 if not must and not flt else 0)
            return self.node(must + must_not + flt + should, msm)
        raise N.SlgError(N.ERR_INVALID, f"unknown matcher kind {kind!r}")


def compile_matchers(queries, n_segs):
    """queries: one description per query (None: no matcher) -> the dict of GpuIndex.search_batch_bool_tree:
    c_offsets, c_terms [total, n_segs], c_group, g_offsets, f_offsets, f_filter, n_offsets, n_min_should, e_offsets,
    e_child, e_kind (slg_bool_tree_spec)."""
    c_offsets, c_terms, c_group, g_offsets = [0], [], [], [0]
    f_offsets, f_filter, n_offsets, n_min_should, e_offsets, e_child, e_kind = [0], [], [0], [], [0], [], []
    for d in queries:
        if d is not None:
            q = _Query(n_segs)
            top = q.walk(d)
            if top[0] == "t":  # a matcher that is one term group: one node with that leaf as its MUST child
                q.node([(top, MUST)], 0)
            ng, nl = len(q.groups), len(q.groups) + len(q.filters)
            index = {"t": 0, "f": ng, "n": nl}
            for g, terms in enumerate(q.groups):
                c_terms.extend(terms)
                c_group.extend([g] * len(terms))
            f_filter.extend(q.filters)
            for edges, ms in q.nodes:
                n_min_should.append(ms)
                for (what, i), kind in edges:
                    e_child.append(index[what] + i)
                    e_kind.append(kind)
                e_offsets.append(len(e_child))
            g_offsets.append(g_offsets[-1] + ng)
        else:
            g_offsets.append(g_offsets[-1])
        c_offsets.append(len(c_group))
        f_offsets.append(len(f_filter))
        n_offsets.append(len(n_min_should))
    u32 = lambda a: np.array(a, np.uint32)
    return dict(c_offsets=u32(c_offsets), c_terms=u32(c_terms).reshape(-1, n_segs), c_group=u32(c_group),
                g_offsets=u32(g_offsets), f_offsets=u32(f_offsets), f_filter=np.array(f_filter, np.int32),
                n_offsets=u32(n_offsets), n_min_should=u32(n_min_should), e_offsets=u32(e_offsets),
                e_child=u32(e_child), e_kind=np.array(e_kind, np.int32))
