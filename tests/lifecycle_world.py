"""A model of an updatable index for the lifecycle tests: plain data and references, no device.

The index state machine (searchlite_amd/csrc/slg_index.hip: update_state, copy_state, reshape_per_segment,
finish_state, slg_index_update_deleted / _add_segment / _remove_segment) keeps one entry PER SEGMENT of every registered
resource and rebuilds each state's device tables from them.  The Model below is the same thing as parallel Python
lists, one entry per segment:

    segs   the Segment: postings, tombstones (`deleted`, `docs`), positions, the embedded vector store
    tok    the token sequences the segment was built from (what a compaction merges)
    keys   the term dictionary, "field:term" by term id (slg_index_set_terms)
    mask   the pass mask of the bitmap filter (add_filter)
    rcol   the i64 column of the range filter (add_filter_range, LO <= v <= HI)
    num    the numeric agg column, i64 value lists per doc (ranked: cardinality and percentiles read its ranks)
    kw     the keyword agg column, ordinals into KEYS, at most one per doc (terms aggregations, collapse, the leaf of
           the tree filter)
    si/sf  the i64 and the f64 sort field, value lists per doc
    xvec   the store of the extra vector field, (metric, offsets, values) or None
    text   the stored texts of the text field, ASCII bytes per doc (built from tok; a few empty), or None: the
           segment has no text at all (add_text_field with NULL offsets)
    npath  the nested paths c and c.r (c.r bound to c): {"counts": {path: objects per doc}, "parents": {"c.r": the
           parent index of every reply, or None}}, as tests/nested_ref.py takes them (add_nested_path)
    ncol   the nested value columns c.author (keyword) and c.r.n (i64): values per object per doc (add_nested_*field)
    ts     the i64 timestamp column of the date aggregations, 0 - 2 values per doc around the epoch
The term filter (add_filter_terms) reads the posting lists of TERM_FILTER, the tree filter (add_filter_trees) the kw and
num columns, the nested tree (add_nested_filter_trees: NESTED_FILTER) npath, ncol and kw: their bitmaps derive from the
lists above.  The suggester's doc frequencies derive from segs and keys; `numf`, the f64 column the composite's
histogram source reads, is the num list registered a second time.

delete / add / remove are list operations.  expect(model, kind) gives the expected result of ONE small request of a
kind, from the CPU oracle and the existing restatements only (bool_ref, booltree_ref, phrase_ref, fscore_ref,
script_ref, scan_ref, agg_ref, agg_values_ref, collapse_ref, rescore_ref, expand_ref, hybrid_ref, filter_ref,
agg_date_ref, top_hits_ref, composite_ref, term_buckets_ref, request_ref, nested_ref, regex_ref, suggest_ref,
highlight_ref, and the sort / cursor key helpers and the vector reference of the sort, cursor and vector-search
tests).  request(model, kind,
ids) is the same request as the device takes it, with the ids a live index handed out.

Sizes: 65, 300, 33 and 200 docs put 32 / 33, 64 / 65 and a non-multiple of 32 on the word edges of the tombstone and
reject bitmaps; a fifth segment of 64 docs is appended, a merged one replaces two old ones.  Nothing here is a
workload size on purpose: these are the smallest shapes at which a per-segment table can be wrong.

unshifted(model_before, seg, resource): the model after remove(seg) with ONE resource list left as a library would
leave it that forgot to erase its entry (the would-it-notice argument of tests/test_lifecycle_world.py)."""
import copy

import numpy as np

from searchlite_amd import _native as N
from searchlite_amd import aggs as A
from searchlite_amd import booltree as BT
from searchlite_amd.script import compile_script
from tests import agg_ref, agg_values_ref as V
from tests import bool_ref as B
from tests import agg_date_ref as D
from tests import booltree_ref, collapse_ref, filter_ref, fscore_ref, hybrid_ref, rescore_ref, scan_ref, script_ref
from tests import composite_ref, highlight_ref, nested_ref, request_ref, term_buckets_ref
from tests import top_hits_ref as T
from tests import top_hits_world as TW
from tests import nested_world as NW
from tests import regex_util as X
from tests import suggest_worlds as SW
from tests import collapse_world as CW
from tests import expand_util as U
from tests import phrase_ref as P
from tests.expand_worlds import word
from tests.test_gpu_composite import want_page as want_composite_page
from tests.test_gpu_cursor import cursor_of, key_of, ordered_rows
from tests.test_gpu_phrase import specs_of
from tests.test_gpu_sort import expected_rows
from tests.test_gpu_vector_search import boundary_gap, reference as vector_reference
from tests.util import oracle_rerank_segments

F32 = np.float32
NOVEC = 0xFFFFFFFF
SIZES = (65, 300, 33, 200)
FIFTH = 64
VOCAB = 40
DIM = 16
NQ = 4           # text queries
NV = 4           # queries of the vector-only kind
K, K_PLAIN = 11, 65
KEYS = [f"key{i}" for i in range(6)]
LO, HI = 20, 70                      # the range filter over rcol
TERM_FILTER = (9, 13)                # add_filter_terms: the docs that hold neither
TREE = dict(ords=[1, 4], lo=-10, hi=25)   # the tree filter: kw in {key1, key4} OR -10 <= num <= 25
SORT = [("si", "asc"), ("sf", "desc"), ("_score", "desc")]
PAGE = 5                             # cursor: the page-2 batch starts behind row PAGE - 1
COLLAPSE = dict(group_limit=5, inner_from=0, inner_size=3)
INNER_SORT = [("si", "asc")]
CAND, K_OUT = 20, 11
# the first seed from 20270 on whose world passes tests/test_lifecycle_world.py: with four queries, a hit of every kind
# in every segment that a step touches and the vector kinds' near-tie gaps are what most seeds miss
SEED = 20296
RESOURCES = ("keys", "mask", "rcol", "num", "kw", "si", "sf", "xvec", "positions", "f_terms", "f_tree",
             "text", "npath", "ncol", "ts", "f_nested")
# canonical ids: what a fresh index hands out when everything is registered in the order of
# tests/test_gpu_lifecycle.py: Live.register
CANON = dict(num=0, kw=1, f_mask=0, f_range=1, f_terms=2, f_tree=3, si=0, sf=1, xvec=1,
             ts=2, numf=3, text=0, p_c=0, p_cr=1, n_author=0, n_n=1, f_nested=4)
# the kinds the suite was written with: the tombstone sets are drawn from THEIR hits, so they stay what they were
OLD_KINDS = ("plain", "sorted", "cursor", "bool", "tree", "phrase", "fscore", "script", "scan", "aggs", "collapse",
             "rescore", "expand", "vector", "hybrid", "rerank")
KINDS = OLD_KINDS + ("date_aggs", "top_hits", "composite", "term_buckets", "request", "nested", "regex", "suggest",
                    "highlight", "highlight_batch")
PREPARED = ("plain", "sorted", "cursor", "bool", "tree", "phrase", "fscore", "script", "scan", "aggs", "collapse",
            "rescore", "date_aggs", "top_hits", "composite", "term_buckets", "request")
# what a kind reads of the registered resources (the segments themselves are read by all)
READS = {
    "plain": (), "rescore": (),
    "sorted": ("si", "sf"), "cursor": ("si", "sf"),
    "bool": ("mask", "rcol", "f_terms", "f_tree"),
    "tree": ("f_tree",),
    "phrase": ("positions",),
    "fscore": ("num", "mask"), "script": ("num",),
    "scan": ("num", "mask", "rcol", "f_terms", "f_tree"),
    "aggs": ("num", "kw"),
    "collapse": ("kw", "si"),
    "expand": ("keys",),
    "vector": ("xvec",), "hybrid": ("xvec",), "rerank": ("xvec",),
    "date_aggs": ("ts", "num", "f_tree"),
    "top_hits": ("kw", "si"), "composite": ("kw", "num"), "term_buckets": ("kw", "mask"),
    "request": ("num", "mask", "kw", "si", "sf"),
    "nested": ("npath", "ncol", "kw", "f_nested"),
    "regex": ("keys",), "suggest": ("keys",),
    "highlight": ("text",), "highlight_batch": ("text",),
}
# tombstones change no dictionary, and a rerank scores the candidates it is handed, deleted or not; the header says
# the same of the regex expansion ("slg_index_update_deleted keeps the dictionaries"), of the suggester
# ("slg_index_update_deleted never changes an answer") and of the texts ("leaves them alone": host hits name their docs)
SAME_UNDER_DELETE = ("expand", "rerank", "regex", "suggest", "highlight")
EDGE_DOCS = (0, 31, 32, 63, 64)


# ---- the model -------------------------------------------------------------------------------------------------
class Model:
    LISTS = ("segs", "tok", "keys", "mask", "rcol", "num", "kw", "si", "sf", "xvec", "text", "npath", "ncol", "ts")

    def __init__(self, queries, **lists):
        self.q = queries           # what the requests are made of: the same for every state of the index
        for name in self.LISTS:
            setattr(self, name, list(lists[name]))
        self._memo = {}
        # derived bitmaps a wrong library could leave behind: None = derive them from the lists
        self.stale = {}

    @property
    def n_segs(self):
        return len(self.segs)

    def clone(self):
        m = Model(self.q, **{name: getattr(self, name) for name in self.LISTS})
        m.stale = dict(self.stale)
        return m

    def entry(self, s):
        """segment s as add() takes it"""
        return {name: getattr(self, name)[s] for name in self.LISTS}

    # -- the steps ---------------------------------------------------------------------------------------------
    def delete(self, seg, docs):
        """new tombstones on top of the segment's (the set only grows) -> (complete bitmap, live docs)"""
        s = copy.copy(self.segs[seg])
        s.set_deleted(sorted(int(d) for d in docs))
        self.segs[seg] = s
        self._memo = {}
        return s.deleted, s.docs

    def add(self, entry):
        for name in self.LISTS:
            getattr(self, name).append(entry[name])
        self._memo = {}
        return self.n_segs - 1

    def remove(self, seg):
        for name in self.LISTS:
            del getattr(self, name)[seg]
        self._memo = {}

    # -- views -------------------------------------------------------------------------------------------------
    def dead(self, s):
        seg = self.segs[s]
        if seg.deleted is None:
            return np.zeros(seg.n_docs, bool)
        return np.unpackbits(np.asarray(seg.deleted, np.uint8), bitorder="little")[:seg.n_docs].astype(bool)

    def n_docs(self):
        return [int(s.n_docs) for s in self.segs]

    def filter_masks(self):
        """pass masks per filter name (tombstones not applied), as the four constructors build them"""
        if "filters" in self._memo:
            return self._memo["filters"]
        out = {"f_mask": [np.asarray(m, bool) for m in self.mask],
               "f_range": [(np.asarray(c) >= LO) & (np.asarray(c) <= HI) for c in self.rcol]}
        terms = []
        for seg in self.segs:
            held = np.zeros(seg.n_docs, bool)
            for t in TERM_FILTER:
                held[B.postings(seg, t)] = True
            terms.append(~held)
        out["f_terms"] = terms
        nodes, ords = tree_program(CANON)
        by_id = {CANON["kw"]: dict(kind="keyword", keys=KEYS, docs=self.kw, id=CANON["kw"]),
                 CANON["num"]: dict(kind="i64", keys=None, docs=self.num, id=CANON["num"])}
        out["f_tree"] = [filter_ref.eval_program(nodes, ords, by_id, {}, s, seg.n_docs) for s, seg in enumerate(self.segs)]
        out["f_nested"] = [np.array(nested_ref.mask(nested_world(self, s), NESTED_FILTER), bool) for s in range(self.n_segs)]
        for name, masks in self.stale.items():  # (a bitmap list a wrong library left unshifted)
            if name in out:
                out[name] = [fit(m, seg.n_docs) for m, seg in zip(masks, self.segs)]
        self._memo["filters"] = out
        return out

    def filters_by_id(self, ids=CANON):
        fm = self.filter_masks()
        return {ids[name]: fm[name] for name in ("f_mask", "f_range", "f_terms", "f_tree", "f_nested")}

    def vector_fields(self):
        """[embedded store per segment, extra field per segment] as (metric, offsets, values) or None"""
        emb = [None if s.vec_values is None else (int(s.vec_metric), s.vec_offsets, s.vec_values) for s in self.segs]
        return [emb, list(self.xvec)]


def fit(values, n):
    """another segment's per-doc array read with this segment's n docs: cut, or repeated, to n entries"""
    if values is None:
        return None
    if isinstance(values, np.ndarray):
        return np.resize(values, n) if len(values) else np.zeros(n, values.dtype)
    return [values[d % len(values)] for d in range(n)] if len(values) else [[] for _ in range(n)]


def unshifted(before, seg, resource):
    """`before` after remove(seg), but with `resource` as a library would leave it that shrank the segment list and
    not this resource's list: entry i of the resource stays with ordinal i.  Removing the LAST segment that way
    gives the right answer by construction, so there the slip modelled is the other one-line slip, erasing the first
    entry instead.  Per-doc arrays of another segment are cut or repeated to the segment's docs (fit)."""
    m = before.clone()
    m.remove(seg)
    n = m.n_segs
    last = seg == before.n_segs - 1
    keep = (lambda lst: list(lst[1:])) if last else (lambda lst: list(lst[:n]))
    if resource == "positions":
        old = keep([(s.pos_offsets, s.positions, s) for s in before.segs])
        for i, (po, ps, src) in enumerate(old):
            s = copy.copy(m.segs[i])
            # positions are per posting: another segment's arrays, cut or repeated to this segment's postings
            cnt = np.diff(po.astype(np.int64))
            cnt = np.resize(cnt, s.n_postings) if len(cnt) else np.zeros(s.n_postings, np.int64)
            offs = np.zeros(s.n_postings + 1, np.uint64)
            np.cumsum(cnt, out=offs[1:])
            s.pos_offsets, s.positions = offs, np.resize(ps, int(offs[-1])).astype(np.uint32)
            m.segs[i] = s
    elif resource in ("f_terms", "f_tree", "f_nested"):
        m.stale[resource] = keep(before.filter_masks()[resource])
    elif resource == "npath":
        m.npath = [{part: {p: fit(v, sg.n_docs) for p, v in old[part].items()} for part in ("counts", "parents")}
                   for old, sg in zip(keep(before.npath), m.segs)]
    elif resource == "ncol":
        m.ncol = [{name: fit(v, sg.n_docs) for name, v in old.items()} for old, sg in zip(keep(before.ncol), m.segs)]
    elif resource == "keys":
        m.keys = keep(before.keys)
    elif resource == "xvec":
        old = keep(before.xvec)
        m.xvec = [None if st is None else (st[0], fit(st[1], sg.n_docs), st[2]) for st, sg in zip(old, m.segs)]
    else:
        old = keep(getattr(before, resource))
        setattr(m, resource, [fit(v, sg.n_docs) for v, sg in zip(old, m.segs)])
    m._memo = {}
    return m


# ---- building the world ------------------------------------------------------------------------------------------
def _unit(rng, n, dim):
    v = rng.standard_normal((n, dim)).astype(F32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True).astype(F32)).astype(F32)


def _store(rng, n_docs, toward=None, p_missing=0.2):
    """a cosine store: some docs without a vector, rows out of doc order; toward: query vectors [nq, DIM] the rows
    lean to (a small segment's docs then rank among the first hits of the vector kinds)"""
    have = rng.random(n_docs) >= p_missing
    rows = int(have.sum())
    offs = np.full(n_docs, NOVEC, np.uint32)
    offs[np.nonzero(have)[0]] = rng.permutation(rows)
    vals = _unit(rng, max(rows, 1), DIM)
    if toward is not None:
        vals = (F32(0.5) * toward[np.arange(len(vals)) % len(toward)] + F32(0.85) * vals).astype(F32)
        vals = (vals / np.linalg.norm(vals, axis=1, keepdims=True).astype(F32)).astype(F32)
    return 0, offs, vals


def segment_of(tok, store):
    """the Segment of token sequences (postings, tfs and positions agree) with its embedded vector store"""
    seg = P.segment_from_tokens(tok, VOCAB, k1=0.9, b=0.4)
    seg.vec_dim, seg.vec_metric, seg.vec_offsets, seg.vec_values = DIM, store[0], store[1], store[2]
    return seg


def make_entry(rng, n, key_words, qv, shuffle_keys=False, extra_vectors=True):
    """one segment of n docs with the source data of every resource; the docs of a small segment are short, so that
    they rank among every query's first hits, and their sort values lie at the front of both sort orders (a step
    on a small segment then shows in every kind)"""
    lo, hi = (3, 8) if n < 100 else (6, 15)
    si_hi, sf_lo = (3, 20) if n < 100 else (8, -40)
    p = 1.0 / np.arange(1, VOCAB + 1)
    p /= p.sum()
    tok = [rng.choice(VOCAB, size=int(rng.integers(lo, hi)), p=p).tolist() for _ in range(n)]
    for t in range(VOCAB):  # every term has a posting: the dictionary and the postings agree on the vocabulary
        tok[int(rng.integers(0, n))].append(t)
    keys = ["body:" + word(int(i)) for i in sorted(key_words)]
    if shuffle_keys:
        keys = [keys[i] for i in rng.permutation(len(keys))]   # term ids against the byte order
    return dict(
        segs=segment_of(tok, _store(rng, n, qv[:, :DIM] if n < 100 else None)), tok=tok, keys=keys,
        mask=rng.random(n) < 0.6,
        rcol=rng.integers(0, 100, n).astype(np.int64),
        num=[[int(x) for x in rng.integers(-50, 51, int(rng.integers(0, 3)))] for _ in range(n)],
        kw=[[int(rng.integers(0, len(KEYS)))] if rng.random() < 0.85 else [] for _ in range(n)],
        si=[[int(x) for x in rng.integers(0, si_hi, int(rng.integers(0, 3)))] for _ in range(n)],
        sf=[[float(x) / 4.0 for x in rng.integers(sf_lo, 40, int(rng.integers(0, 3)))] for _ in range(n)],
        xvec=_store(rng, n, qv[:, DIM:] if n < 100 else None, p_missing=0.3) if extra_vectors else None)


# ---- the lists of the resources added since: a random stream of their own, so that every draw above stays what it was
MORE_SEED = 20261020
DAY = 86_400_000
AUTHORS = ["a0", "a1", "a2"]
NESTED_KEY = 5                       # the doc-level leaf of the nested tree: kw == KEYS[NESTED_KEY]
N_LO, N_HI = -1, 2                   # ... and its innermost leaf: a reply's n in [N_LO, N_HI]
NESTED_FILTER = NW.AND(NW.nest("c", NW.keq("author", "a0")), NW.nest("c", NW.nest("r", NW.i64("n", N_LO, N_HI))),
                       NW.keq("kw", KEYS[NESTED_KEY]))
NESTED_KINDS = {"kw": "keyword", "c.author": "keyword", "c.r.n": "i64"}
TEXTLESS = 3                         # the segment whose text field has no text at all (NULL offsets)
SEPARATORS = (" ", " ", ", ", " - ", ". ")


def tword(t):
    """the word a token id stands for in the stored texts (one vocabulary for every segment)"""
    return word(int(t))


def text_of(rng, tokens):
    """a doc's stored text: its token sequence as words, some capitalised (the match folds ASCII case), with mixed
    separators between them"""
    words = [tword(t).capitalize() if rng.random() < 0.2 else tword(t) for t in tokens]
    out = words[0]
    for w in words[1:]:
        out += SEPARATORS[int(rng.integers(0, len(SEPARATORS)))] + w
    return out.encode("ascii")


def crosses_a_word(counts):
    """the docs whose object range [first, first + count) lies in two 32-bit words of the object bitmap"""
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return [d for d, (f, c) in enumerate(zip(first, counts)) if c and f // 32 != (f + c - 1) // 32]


def make_more(rng, n, tok, kw, textless=False):
    """the lists of one segment for the text field, the two nested paths (c, and c.r bound to it), the two nested
    columns (c.author keyword, c.r.n i64) and the timestamp column.  Object counts per doc come from {0, 1, 2, 5}; in
    a segment of 64 docs or more some doc's objects cross a 32-bit word.  The docs whose kw is KEYS[NESTED_KEY] mostly
    hold an object that passes the nested leaves (a0, with a reply bound to it whose n is in range): the tree then
    passes a few docs of every segment, and every other doc fails it"""
    pick = lambda: int((0, 1, 2, 5)[int(rng.integers(0, 4))])
    while True:
        c = [pick() for _ in range(n)]
        if n < 64 or crosses_a_word(c):
            break
    r = [pick() for _ in range(n)]
    parents, author, nn = [], [], []
    for d in range(n):
        row = [None if rng.random() < 0.1 or c[d] == 0 else int(rng.integers(0, c[d])) for _ in range(r[d])]
        a = [[AUTHORS[int(rng.integers(0, len(AUTHORS)))]] if rng.random() < 0.8 else [] for _ in range(c[d])]
        v = [[int(rng.integers(-4, 5))] if rng.random() < 0.8 else [] for _ in range(r[d])]
        if kw[d] == [NESTED_KEY] and (rng.random() < 0.9 or d in EDGE_DOCS):
            c[d], r[d] = max(c[d], 1), max(r[d], 1)
            a, row, v = (a or [[]]), (row or [None]), (v or [[]])
            o = int(rng.integers(0, c[d]))
            a += [[] for _ in range(c[d] - len(a))]
            a[o], row[-1], v[-1] = ["a0"], o, [int(rng.integers(N_LO, N_HI + 1))]
        for objs in (a, v):                               # padded only up to the last object that had a value
            while objs and not objs[-1]:
                objs.pop()
        parents.append(row)
        author.append(a)
        nn.append(v)
    if n >= 64 and not crosses_a_word(c):                 # (the forced objects moved the ranges: draw again)
        return make_more(rng, n, tok, kw, textless)
    ts = []
    for d in range(n):
        u = rng.random()
        ts.append([] if u < 0.1 else [int(x) for x in rng.integers(-40 * DAY, 40 * DAY, 2 if u < 0.2 else 1)])
    ts[1], ts[2] = [-1], [0, 31 * DAY]                    # the last ms of 1969 and the first of 1970 and of its February
    text = None if textless else [b"" if d % 13 == 5 else text_of(rng, tok[d]) for d in range(n)]
    return dict(text=text, ts=ts, npath=dict(counts={"c": c, "c.r": r}, parents={"c.r": parents}),
                ncol={"c.author": author, "c.r.n": nn})


def nested_world(m, s):
    """segment s as tests/nested_ref.py takes it"""
    return {"n_docs": int(m.segs[s].n_docs), "kinds": NESTED_KINDS, "doc": {"kw": [[KEYS[o] for o in d] for d in m.kw[s]]},
            "counts": m.npath[s]["counts"], "parents": m.npath[s]["parents"], "nested": m.ncol[s]}


def merge_entries(a, b):
    """the segment a compaction writes for a and b: the docs of a, then the docs of b, tombstones gone (every
    per-doc resource concatenated; the postings keep the token ids, so the dictionary is a's, key by term id)"""
    na = a["segs"].n_docs
    tok = a["tok"] + b["tok"]
    ea = (a["segs"].vec_metric, a["segs"].vec_offsets, a["segs"].vec_values)
    eb = (b["segs"].vec_metric, b["segs"].vec_offsets, b["segs"].vec_values)

    def cat_store(x, y, ny):
        if x is None and y is None:
            return None
        dim_of = (x or y)[2].shape[1]
        xo = np.full(na, NOVEC, np.uint32) if x is None else x[1]
        xv = np.zeros((0, dim_of), F32) if x is None else x[2]
        yo = np.full(ny, NOVEC, np.uint32) if y is None else y[1]
        yv = np.zeros((0, dim_of), F32) if y is None else y[2]
        yo = np.where(yo == NOVEC, NOVEC, yo.astype(np.int64) + len(xv)).astype(np.uint32)
        return (x or y)[0], np.concatenate([xo, yo]), np.concatenate([xv, yv]).astype(F32)

    nb = b["segs"].n_docs
    texts = lambda e, n: [b""] * n if e["text"] is None else e["text"]
    more = dict(
        text=None if a["text"] is None and b["text"] is None else texts(a, na) + texts(b, nb), ts=a["ts"] + b["ts"],
        npath={part: {p: a["npath"][part][p] + b["npath"][part][p] for p in a["npath"][part]} for part in ("counts", "parents")},
        ncol={name: a["ncol"][name] + b["ncol"][name] for name in a["ncol"]})
    return dict(
        more,
        segs=segment_of(tok, cat_store(ea, eb, nb)), tok=tok,
        keys=list(a["keys"]),
        mask=np.concatenate([a["mask"], b["mask"]]), rcol=np.concatenate([a["rcol"], b["rcol"]]),
        num=a["num"] + b["num"], kw=a["kw"] + b["kw"], si=a["si"] + b["si"], sf=a["sf"] + b["sf"],
        xvec=cat_store(a["xvec"], b["xvec"], nb))


def make_queries(rng):
    """the request data every kind draws on; term ids are the same in every segment (one vocabulary)"""
    hot = np.arange(14)
    offs, terms = [0], []
    for q in range(NQ - 1):
        terms += rng.choice(hot, size=3, replace=False).tolist()
        offs.append(len(terms))
    terms += rng.choice(VOCAB, size=12, replace=False).tolist()   # the many-term query: 12 lists
    offs.append(len(terms))
    w = (rng.random(len(terms)) * 2 + 0.25).astype(F32)
    r_terms = rng.choice(hot, size=2 * NQ).astype(np.uint32)
    qv = np.concatenate([_unit(rng, NQ, DIM), _unit(rng, NQ, DIM)], axis=1)
    return dict(
        offs=np.array(offs, np.uint32), terms=np.array(terms, np.uint32), w=w,
        p_terms=[(q % 5, (q + 1) % 5) for q in range(NQ)],
        r_offs=(np.arange(NQ + 1) * 2).astype(np.uint32), r_terms=r_terms,
        r_w=(rng.random(2 * NQ) + 0.5).astype(F32),
        qv=qv, alpha=rng.choice(np.array([0.0, 0.3, 0.5, 0.8], F32), size=(NQ, 2)).astype(F32),
        boost=(rng.random((NQ, 2)) + 0.5).astype(F32),
        cand_perm=[rng.permutation(400) for _ in range(NQ)], cand_bm=(rng.random((NQ, 64)) * 5).astype(F32))


_world = {}


def build(seed=SEED):
    """-> (the four-segment model, the fifth segment's entry).  Tombstones already in segments 1 and 3, `deleted`
    null in 0 and 2; segment 1's term ids are a shuffle of the byte order, and it has no vectors in the extra field.  Built once per seed; callers get clones."""
    if seed not in _world:
        rng = np.random.default_rng(seed)
        pools = [rng.choice(120, size=VOCAB, replace=False) for _ in range(len(SIZES) + 1)]
        queries = make_queries(rng)
        entries = [make_entry(rng, n, pools[i], queries["qv"], shuffle_keys=i == 1, extra_vectors=i != 1)
                   for i, n in enumerate(SIZES)]
        fifth = make_entry(rng, FIFTH, pools[-1], queries["qv"])
        more = np.random.default_rng(MORE_SEED)   # (the new lists draw from a stream of their own)
        for i, e in enumerate(entries + [fifth]):
            e.update(make_more(more, e["segs"].n_docs, e["tok"], e["kw"], textless=i == TEXTLESS))
        # the first and the last segment each hold an end of the numeric column's value range alone: removing one
        # shrinks the dense id range of a histogram over the column (what the field records of its values must follow)
        entries[0]["num"][5], entries[3]["num"][7] = [90], [-90]
        m = Model(queries, **{name: [e[name] for e in entries] for name in Model.LISTS})
        m.q["x_words"] = (entries[0]["keys"][3].split(":", 1)[1], entries[3]["keys"][7].split(":", 1)[1])
        m.delete(1, np.nonzero(rng.random(SIZES[1]) < 0.1)[0])
        m.delete(3, np.nonzero(rng.random(SIZES[3]) < 0.15)[0].tolist() + [SIZES[3] - 1])
        _world[seed] = (m, fifth)
    m, fifth = _world[seed]
    return m.clone(), dict(fifth)


def _with_hits(m, seg, docs, oracle):
    """docs plus, for every kind a delete must show in, the first doc of segment `seg` among the rows its device
    check compares: the tombstones then remove a current hit of every kind"""
    out = set(docs)
    for kind in OLD_KINDS:   # (the kinds added since show a delete through these docs: tests/test_lifecycle_world.py)
        if kind in SAME_UNDER_DELETE:
            continue
        hit = [d for s, d in hit_docs(m, kind, oracle) if s == seg]
        assert hit, f"{kind} has no hit in segment {seg}: a delete there could not show in it"
        out.add(hit[0])
    return sorted(out)


def tombstone_sets(m, oracle=None):
    """the delete scenario's three steps, as (segment, docs), each drawn on the state the one before leaves: the
    edge docs and a current hit of every kind of the 65-doc segment; a larger set on the same segment (every third doc too);
    every doc of the 33-doc segment"""
    oracle = the_oracle() if oracle is None else oracle
    m = m.clone()
    first = _with_hits(m, 0, set(EDGE_DOCS), oracle)
    m.delete(0, first)
    second = _with_hits(m, 0, set(first) | set(range(1, SIZES[0], 3)), oracle)
    return [(0, first), (0, second), (2, list(range(SIZES[2])))]


def shifted_tombstones(m, oracle=None):
    """for the model after remove(0): tombstones on ordinal 1, the 33-doc segment that used to be ordinal 2"""
    assert m.n_docs()[1] == SIZES[2]
    return 1, _with_hits(m, 1, {0, 31, 32}, the_oracle() if oracle is None else oracle)


# ---- the scenarios, as steps on the model (tests/test_gpu_lifecycle.py applies the same steps to a live index) ----
SCENARIOS = ("delete", "remove_first", "remove_middle", "remove_last", "remove_then_delete", "add", "compaction")


def scenario(name, seed=SEED):
    """-> (the starting model, [(label, op)]); op = ("delete", seg, docs) | ("add", entry) | ("remove", seg)"""
    m, fifth = build(seed)
    if name == "delete":
        return m, [(f"tombstones {i}", ("delete", seg, docs)) for i, (seg, docs) in enumerate(tombstone_sets(m))]
    if name.startswith("remove_") and name != "remove_then_delete":
        seg = {"first": 0, "middle": 1, "last": len(SIZES) - 1}[name.split("_", 1)[1]]
        return m, [(f"remove {seg}", ("remove", seg))]
    if name == "remove_then_delete":
        after = m.clone()
        after.remove(0)
        seg, docs = shifted_tombstones(after)
        return m, [("remove 0", ("remove", 0)), (f"tombstones on the new ordinal {seg}", ("delete", seg, docs))]
    if name == "add":
        return m, [("add the fifth", ("add", fifth))]
    if name == "compaction":
        # segments 0 and 2 become one: add the merged segment, drop the old ones (the second at its shifted ordinal)
        return m, [("add the merged", ("add", merge_entries(m.entry(0), m.entry(2)))), ("remove 0", ("remove", 0)),
                   ("remove 1 (was 2)", ("remove", 1))]
    raise ValueError(name)


def apply(m, op):
    if op[0] == "delete":
        return m.delete(op[1], op[2])
    if op[0] == "add":
        return m.add(op[1])
    return m.remove(op[1])


# ---- requests --------------------------------------------------------------------------------------------------
def text_queries(m):
    q = m.q
    return q["offs"], np.repeat(q["terms"][:, None], m.n_segs, axis=1).astype(np.uint32), q["w"]


def tree_program(ids):
    """the tree filter as slg_index_add_filter_trees takes it: kw in TREE.ords OR lo <= num <= hi"""
    nodes = [dict(kind=N.FILTER_KEYWORD_IN, field=ids["kw"], ord_begin=0, n_ords_in=len(TREE["ords"])),
             dict(kind=N.FILTER_RANGE_I64, field=ids["num"], lo_i=TREE["lo"], hi_i=TREE["hi"]),
             dict(kind=N.FILTER_OR, arity=2)]
    return nodes, list(TREE["ords"])


def term_filter_rows(m):
    return np.repeat(np.array(TERM_FILTER, np.uint32)[:, None], m.n_segs, axis=1)


def sort_ids(sort, ids):
    return [(p if p == "_score" else ids[p], o) for p, o in sort]


FILTER_CYCLE = ("f_mask", "f_range", "f_terms", "f_tree")


def bool_queries():
    return [([(B.MUST, [q % 4]), (B.SHOULD, [4 + q % 3]), (B.MUST_NOT, [8 + q % 2])], 0) for q in range(NQ)]


def tree_descs(ids):
    T = lambda *t: {"term": list(t)}
    return [{"bool": {"must": [T(q % 3)], "filter": [ids["f_tree"]],
                      "should": [T(4), {"dis_max": [T(6), T(7 + q % 2)]}], "minimum_should_match": q % 2}}
            for q in range(NQ)]


def phrase_queries(m):
    """(scored queries, clauses, phrases): query q must hold its two terms within slop 2 of each other"""
    pt = m.q["p_terms"]
    offs = (np.arange(NQ + 1) * 2).astype(np.uint32)
    terms = np.repeat(np.array([t for pair in pt for t in pair], np.uint32)[:, None], m.n_segs, axis=1)
    w = np.tile(np.array([1.0, 0.5], F32), NQ)
    cl, ph = specs_of([([], [(P.MUST, 2, [[a, b]])], 0) for a, b in pt], m.n_segs)
    return (offs, terms, w), cl, ph


def fscore_functions(ids):
    fvf = dict(kind="field_value_factor", field=ids["num"], modifier="sqrt", factor=0.5, missing=2.0)
    wt = dict(kind="weight", weight=1.5, filter=ids["f_mask"])
    return [dict(functions=[fvf, wt], score_mode="sum", boost_mode="sum" if q % 2 else "multiply") for q in range(NQ)]


def scripts(ids):
    return [dict(program=compile_script("_score * 2 + num / 4" if q % 2 else "num - _score", None, {"num": ids["num"]}),
                 boost=1.0 if q % 4 else -1.5) for q in range(NQ)]


def scan_queries(ids):
    RF = lambda **kw: {"rank_feature": dict(field=ids["num"], **kw)}
    qs = [RF(modifier="sqrt", boost=2.0), RF(boost=-0.5, missing=3.0), RF(modifier="reciprocal", boost=3.0),
          {"match_all": {}}, {"constant_score": dict(filter=ids["f_range"], boost=1.5)},
          {"constant_score": dict(boost=2.5)}, RF(modifier="sqrt"), RF(missing=-7.0)]
    root = [-1, ids["f_tree"], -1, ids["f_terms"], -1, ids["f_mask"], ids["f_range"], ids["f_tree"]]
    return qs, np.array(root, np.int32)


AGGS = {"t": {"type": "terms", "field": "kw", "aggs": {"c": {"type": "cardinality", "field": "num"}}},
        "h": {"type": "histogram", "field": "num", "interval": 7, "offset": 0.25},
        "s": {"type": "stats", "field": "num"},
        "c": {"type": "cardinality", "field": "num"},
        "p": {"type": "percentiles", "field": "num"}}
KEYS_OF = {"kw": KEYS}


def agg_plan(ids):
    return A.agg_spec(AGGS, {"kw": {"id": ids["kw"], "keys": KEYS}, "num": {"id": ids["num"]}})


def agg_columns(m):
    return {"kw": [[[KEYS[o] for o in d] for d in seg] for seg in m.kw], "num": m.num}


def rescore_spec(m):
    q = m.q
    return dict(q_offsets=q["r_offs"], q_terms=np.repeat(q["r_terms"][:, None], m.n_segs, axis=1).astype(np.uint32),
                q_weights=q["r_w"], window=np.array([7, 11, 3, 20], np.uint32),
                mode=np.array([rescore_ref.TOTAL, rescore_ref.MULTIPLY, rescore_ref.MAX, rescore_ref.MIN], np.int32))


def expand_requests(m):
    """fuzzy, prefix and wildcard in one call, over words some segments hold and others lack"""
    w0, w1 = m.q["x_words"]
    return [U.fuzzy("body", w0, 1, 1, 50, 3), U.fuzzy("body", w1[:3] + "z", 2, 1, 50, 3), U.prefix("body", "aa", 50),
            U.prefix("body", "aab", 7), U.wildcard("body", "a?c*", 50), U.wildcard("body", "*b", 50)]


def vector_request(m, ids, nq=NV):
    q = m.q
    return dict(clause_field=[0, ids["xvec"]], qvecs=q["qv"][:nq], alpha=q["alpha"][:nq], boost=q["boost"][:nq],
                cand=CAND, k_out=K_OUT)


def rerank_queries(m, ids=CANON):
    """per query the dict of tests.util.rerank_exact: up to 8 candidates from every segment"""
    q = m.q
    out = []
    for i in range(NV):
        seg, doc = [], []
        for s, n in enumerate(m.n_docs()):
            d = [int(x) for x in q["cand_perm"][i] if x < n][:8]
            seg += [s] * len(d)
            doc += d
        out.append(dict(cf=[0, ids["xvec"]], qv=[q["qv"][i, :DIM], q["qv"][i, DIM:]], alpha=q["alpha"][i], boost=q["boost"][i],
                        seg=np.array(seg, np.uint32), doc=np.array(doc, np.uint32), bm=q["cand_bm"][i, :len(doc)].copy()))
    return out


def rerank_fields(m):
    """the two vector fields as tests.util.rerank_exact takes them"""
    return [dict(metric=metric, dim=DIM, segs=[None if st is None else (st[1], st[2]) for st in stores])
            for metric, stores in zip((0, 0), m.vector_fields())]


# a calendar-month date_histogram with a stats child, a date_range whose bounds are the epoch and the first of
# February 1970, and a filter aggregation over the registered tree filter
DATE_AGGS = {"h": {"type": "date_histogram", "field": "ts", "calendar_interval": "month",
                   "aggs": {"s": {"type": "stats", "field": "num"}}},
             "r": {"type": "date_range", "field": "ts",
                   "ranges": [{"to": "1970-01-01T00:00:00Z"}, {"from": "0", "to": "1970-02-01T00:00:00Z"},
                              {"from": "1970-02-01T00:00:00Z"}]},
             "f": {"type": "filter", "filter": {"name": "f_tree"}}}


def date_plan(ids, request=DATE_AGGS):
    return A.agg_spec(request, {"ts": {"id": ids["ts"]}, "num": {"id": ids["num"]},
                                  A.FILTERS: lambda body: ids[body["name"]]})


def date_columns(m):
    return {"ts": m.ts, "num": m.num}


def nested_program(ids):
    """the nested tree as slg_index_add_nested_filter_trees takes it, compiled against the ids of a live index"""
    from searchlite_amd.filters import compile_nested_filter
    fields = {"kw": {"id": ids["kw"], "kind": "keyword", "keys": KEYS}}
    nested = {"paths": {"c": {"id": ids["p_c"]}, "c.r": {"id": ids["p_cr"]}},
              "fields": {"c.author": {"id": ids["n_author"], "path": "c", "kind": "keyword", "keys": AUTHORS},
                         "c.r.n": {"id": ids["n_n"], "path": "c.r", "kind": "i64", "keys": None}}}
    return compile_nested_filter(NESTED_FILTER, fields, nested)


def nested_arrays(m):
    """what add_nested_path (c, then c.r) and add_nested_keyword_field / add_nested_field take, per segment"""
    worlds = [nested_world(m, s) for s in range(m.n_segs)]
    for w in worlds:   # (top-level objects carry no parent list: the path is registered with counts alone)
        assert "c" not in w["parents"]
    return dict(c=[NW.path_arrays(w, "c") for w in worlds], cr=[NW.path_arrays(w, "c.r") for w in worlds],
                author=[NW.column_arrays(w, "c.author", AUTHORS) for w in worlds],
                n=[NW.column_arrays(w, "c.r.n") for w in worlds])


def regex_requests(m):
    """one regex per query over the dictionaries: a class after a literal prefix, one of the expansion's own words
    with its last letter open, a suffix (no literal prefix: the whole field is scanned) and an alternation"""
    w0, _ = m.q["x_words"]
    return [X.regex("body", "aa[a-b].*", 50), X.regex("body", w0[:3] + ".", 50), X.regex("body", ".*b", 7),
            X.regex("body", "aab[a-m]|aac.+", 50)]


def suggest_requests(m):
    """a plain prefix and a fuzzy completion: their scores are sums of per-segment doc frequencies"""
    from searchlite_amd.searcher import suggest_request
    return [suggest_request("body", "aab", 5), suggest_request("body", m.q["x_words"][0], 5, {})]


def suggest_segments(m):
    """per segment [(key, doc frequency)] in term-id order, as tests/suggest_worlds.py: World takes them"""
    return [[(k, int(seg.df(t))) for t, k in enumerate(keys)] for seg, keys in zip(m.segs, m.keys)]


def highlight_specs(m, field):
    """per query one spec: the query's third term as a word (of the three positions the one with which every state
    of every scenario has a fragment among the plain batch's rows of each touched segment: the 65-doc segment is down
    to ONE such row after the delete scenario's second step) and its phrase pair as a two-word phrase"""
    from searchlite_amd.highlight import highlight_spec
    q = m.q
    return [[highlight_spec(field, [tword(hl_term(m, i))], [[tword(a), tword(b)]], pre_tag="<b>",
                            post_tag="</b>", fragment_size=24, number_of_fragments=2)]
            for i, (a, b) in enumerate(q["p_terms"])]


def hl_term(m, i):
    return int(m.q["terms"][int(m.q["offs"][i]) + 2])


def highlight_hits(m):
    """host hits that no tombstone moves: per query and segment, in the order of the rerank kind's permutation, the
    first 4 docs whose tokens hold the spec's term and the first 2 that do not"""
    out = []
    for i in range(NQ):
        t, hits = hl_term(m, i), []
        for s, n in enumerate(m.n_docs()):
            docs = [int(x) for x in m.q["cand_perm"][i] if x < n]
            hits += [(s, d) for d in [d for d in docs if t in m.tok[s][d]][:4] + [d for d in docs if t not in m.tok[s][d]][:2]]
        out.append(hits)
    return out


def highlight_items(m, hits, specs):
    """result[q][hit][spec] of tests/highlight_ref.py; a segment without the field's store: SLG_HL_NO_TEXT"""
    return [[[(N.HL_NO_TEXT, []) if m.text[s] is None else (N.HL_OK, highlight_ref.highlight_spec_ref(m.text[s][d], sp))
              for sp in specs[q]] for s, d in hq] for q, hq in enumerate(hits)]


# top_hits: a root node, and a node under a terms parent on kw (a list per key: the many-lists path) sorted by si
TOP_HITS = {"root": {"type": "top_hits", "size": 3, "from": 0, "sort": []},
            "by_kw": {"type": "terms", "field": "kw",
                      "aggs": {"best": {"type": "top_hits", "size": 2, "from": 0, "sort": [{"field": "si", "order": "asc"}]}}}}
# composite: a terms source on kw and a histogram source on num, fewer buckets a page than there are tuples.  The
# header refuses a histogram source over a column registered as i64 ("the reference reads f64 columns only"), so the
# source reads `numf`: the num list registered a second time, as f64 (num_as_f64)
COMPOSITE = {"type": "composite", "size": 4,
             "sources": [{"type": "terms", "name": "kw", "field": "kw"},
                         {"type": "histogram", "name": "num", "field": "numf", "interval": 40}]}
# significant_terms with f_mask as the background filter, and rare_terms.  size = the number of keys and a
# max_doc_count no key exceeds: nothing is truncated or dropped per segment, so term_buckets_ref's per-segment mode
# (the reference, literally) and its all-segment mode (the device's counting) give the same buckets; the background
# counts are in both the sums over the segments in whose foreground the key occurs, of docs that are alive and pass
TERM_BUCKETS = {"sig": {"type": "significant_terms", "field": "kw", "size": len(KEYS), "background_filter": {"name": "f_mask"}},
                "rare": {"type": "rare_terms", "field": "kw", "size": len(KEYS), "max_doc_count": 100000}}


def collector_fields(ids):
    """the `fields` of aggs.agg_spec for the collectors' requests"""
    return {"kw": {"id": ids["kw"], "keys": KEYS}, "num": {"id": ids["num"]}, "numf": {"id": ids["numf"]}, "si": {"sort_id": ids["si"]},
            A.FILTERS: lambda body: ids[body["name"]]}


def num_as_f64(m):
    return [[[float(v) for v in d] for d in seg] for seg in m.num]


def top_hits_plan(ids):
    return A.agg_spec(TOP_HITS, collector_fields(ids))


def composite_plan(ids):
    return A.agg_spec({"cmp": COMPOSITE}, collector_fields(ids))


def term_buckets_plan(ids):
    return A.agg_spec(TERM_BUCKETS, collector_fields(ids))


# the compound request: the bool clause, function_score, the field sort, a terms aggregation and collapse
REQUEST_AGGS = {"t": {"type": "terms", "field": "kw", "aggs": {"s": {"type": "stats", "field": "num"}}}}


def compound_request(m, ids):
    return dict(clauses=B.clauses_of(bool_queries(), m.n_segs), fscore=fscore_functions(ids), sort=sort_ids(SORT, ids),
                aggs=A.agg_spec(REQUEST_AGGS, collector_fields(ids)),
                collapse=dict(COLLAPSE, field=ids["kw"], inner_sort=sort_ids(INNER_SORT, ids)))


def request(m, kind, ids=CANON):
    """the request of `kind` as the device takes it -> dict of keyword arguments (see tests/test_gpu_lifecycle.py)"""
    Q = text_queries(m)
    if kind == "top_hits":
        return dict(q=Q, k=K, aggs=top_hits_plan(ids))
    if kind == "composite":
        return dict(q=Q, k=K, aggs=composite_plan(ids))
    if kind == "term_buckets":
        return dict(q=Q, k=K, aggs=term_buckets_plan(ids))
    if kind == "request":
        return dict(compound_request(m, ids), q=Q, k=K)
    if kind == "date_aggs":
        return dict(q=Q, k=K, aggs=date_plan(ids))
    if kind == "nested":
        qs, _ = scan_queries(ids)
        return dict(filter=ids["f_nested"],
                    bool=dict(q=Q, k=K, clauses=B.clauses_of(bool_queries(), m.n_segs),
                              q_filter=np.full(NQ, ids["f_nested"], np.int32)),
                    scan=dict(queries=qs, k=K, q_filter=np.full(len(qs), ids["f_nested"], np.int32)))
    if kind == "regex":
        return dict(requests=regex_requests(m))
    if kind == "suggest":
        return dict(requests=suggest_requests(m))
    if kind == "highlight":
        return dict(hits=highlight_hits(m), specs=highlight_specs(m, ids["text"]))
    if kind == "highlight_batch":
        return dict(q=Q, k=K_PLAIN, specs=highlight_specs(m, ids["text"]))
    if kind == "plain":
        return dict(q=Q, k=K_PLAIN)
    if kind == "sorted":
        return dict(q=Q, k=K, sort=sort_ids(SORT, ids))
    if kind == "cursor":
        raise ValueError("the cursor request needs the oracle: cursor_request()")
    if kind == "bool":
        return dict(q=Q, k=K, clauses=B.clauses_of(bool_queries(), m.n_segs),
                    q_filter=np.array([ids[FILTER_CYCLE[q % 4]] for q in range(NQ)], np.int32))
    if kind == "tree":
        return dict(q=Q, k=K, clause_tree=BT.compile_matchers(tree_descs(ids), m.n_segs))
    if kind == "phrase":
        pq, cl, ph = phrase_queries(m)
        return dict(q=pq, k=K, clauses=cl, phrases=ph)
    if kind == "fscore":
        return dict(q=Q, k=K, fscore=fscore_functions(ids))
    if kind == "script":
        return dict(q=Q, k=K, script=scripts(ids))
    if kind == "scan":
        qs, root = scan_queries(ids)
        return dict(queries=qs, k=K, q_filter=root)
    if kind == "aggs":
        return dict(q=Q, k=K, aggs=agg_plan(ids))
    if kind == "collapse":
        return dict(q=Q, k=K, collapse=dict(COLLAPSE, field=ids["kw"], inner_sort=sort_ids(INNER_SORT, ids)))
    if kind == "rescore":
        return dict(q=Q, k=K, rescore=rescore_spec(m))
    if kind == "expand":
        return dict(requests=expand_requests(m))
    if kind == "vector":
        return vector_request(m, ids)
    if kind == "hybrid":
        return dict(vector_request(m, ids, NQ), q=Q, k=K, cand=15)
    if kind == "rerank":
        qs = rerank_queries(m, ids)
        width = max(len(x["doc"]) for x in qs)
        pad = lambda a, dt: np.stack([np.concatenate([x[a], np.zeros(width - len(x[a]), dt)]).astype(dt) for x in qs])
        return dict(clause_field=qs[0]["cf"], qvecs=m.q["qv"][:NV], alpha=m.q["alpha"][:NV], boost=m.q["boost"][:NV],
                    cand_doc=pad("doc", np.uint32), cand_seg=pad("seg", np.uint32), cand_bm25=pad("bm", F32),
                    cand_count=np.array([len(x["doc"]) for x in qs], np.uint32), k_out=K_OUT)
    raise ValueError(kind)


# ---- expectations ----------------------------------------------------------------------------------------------
def the_oracle():
    from oracle import oracle as o
    o.build()
    return o


def all_hits(m, oracle):
    if "all" not in m._memo:
        m._memo["all"] = oracle.search_batch(m.segs, *text_queries(m), sum(m.n_docs()), strategy=oracle.BM25)
    return m._memo["all"]


def sort_fields(m):
    return {"si": (m.si, False), "sf": (m.sf, True)}


def cursors_of(m, oracle):
    """-> (every query's hits in SORT order, the cursor behind row PAGE - 1 of each: page 2 starts there)"""
    rows = ordered_rows(all_hits(m, oracle), SORT, sort_fields(m))
    return rows, [cursor_of(hits[PAGE - 1]) if len(hits) >= PAGE else None for hits in rows]


def cursor_request(m, oracle, ids=CANON):
    return dict(q=text_queries(m), k=PAGE + 1, sort=sort_ids(SORT, ids), cursors=cursors_of(m, oracle)[1])


def alive_filters(m, ids=CANON):
    """what a filter leaf reads: the registered bitmap carries its segment's tombstones"""
    return {f: [mk & ~m.dead(s) for s, mk in enumerate(masks)] for f, masks in m.filters_by_id(ids).items()}


def without_registration(m, seg):
    """the model as the device sees segment `seg` between slg_index_add_segment and the second registration, for
    the kinds the header gives an answer (not a refusal) there: no positions (no phrase holds a doc of it), no
    vectors in the extra field and no store in the text field"""
    out = m.clone()
    s = copy.copy(out.segs[seg])
    s.pos_offsets = s.positions = None
    out.segs[seg] = s
    out.xvec[seg] = None
    out.text[seg] = None          # (and no text: SLG_HL_NO_TEXT for its hits)
    return out


def expect(m, kind, oracle=None):
    """the expected result of the kind's request on the model, in the form the kind's own comparison helper takes
    (tests/test_gpu_lifecycle.py: CHECK).  Memoised per model state."""
    if kind not in m._memo:
        m._memo[kind] = _expect(m, kind, the_oracle() if oracle is None else oracle)
    return m._memo[kind]


def _expect_more(m, kind, oracle):
    """the kinds added since, from agg_date_ref, nested_ref (through filter_masks), regex_ref, suggest_ref and
    highlight_ref"""
    Q = text_queries(m)
    segs = m.segs
    if kind == "date_aggs":
        plan, cols = date_plan(CANON), date_columns(m)
        doc, seg, _, count = all_hits(m, oracle)
        docs = [[(int(seg[q, i]), int(doc[q, i])) for i in range(int(count[q]))] for q in range(len(count))]
        layout = D.ref_layout(plan.nodes, cols, KEYS_OF)
        states = [D.run(DATE_AGGS, cols, m.filter_masks(), d) for d in docs]
        per_q = [D.dense(plan.nodes, layout, st, KEYS_OF) for st in states]
        tables = [np.stack([t[i] for t in per_q]) for i in range(len(plan.nodes))]
        return dict(want=(layout, tables, {q: D.respond(DATE_AGGS, st) for q, st in enumerate(states)}), docs=docs,
                    rows=oracle.search_batch(segs, *Q, K, strategy=oracle.BM25))
    if kind == "nested":
        r = request(m, kind)
        filters = m.filters_by_id()
        world = dict(n_docs=m.n_docs(), deleted=[None if s.deleted is None else m.dead(i) for i, s in enumerate(segs)],
                     filters=filters, fields={CANON["num"]: m.num})
        assert not scan_ref.unsafe_docs(r["scan"]["queries"], world)
        rows, matched, _ = scan_ref.search(r["scan"]["queries"], world, K, r["scan"]["q_filter"])
        return dict(bitmaps=alive_filters(m)[CANON["f_nested"]],
                    bool=B.reference(oracle, segs, *Q, K, r["bool"]["clauses"], q_filter=r["bool"]["q_filter"], filters=filters),
                    scan=dict(rows=rows, matched=matched))
    if kind in ("top_hits", "composite", "term_buckets"):
        cols = agg_columns(m)
        hits = TW.hits_of(all_hits(m, oracle))
        docs = [[(s, d) for s, d, _ in h] for h in hits]
        out = dict(matched=[len(h) for h in hits], rows=oracle.search_batch(segs, *Q, K, strategy=oracle.BM25))
        if kind == "top_hits":
            plan = top_hits_plan(CANON)
            layout = D.ref_layout(plan.nodes, cols, KEYS_OF)
            lists, totals = T.expected(TW.ref_nodes(TOP_HITS, plan, layout), layout, hits, cols, m.filter_masks(), KEYS_OF,
                                       sort_fields(m))
            return dict(out, lists=lists, totals=totals)
        if kind == "composite":
            world = dict(cols=dict(cols, numf=num_as_f64(m)), masks={})
            buckets = [composite_ref.collect(COMPOSITE["sources"], world["cols"], ("numf",), d) for d in docs]
            first = [want_composite_page(world, COMPOSITE, b, None) for b in buckets]
            afters = [p.get("after_key") for p in first]
            second = [{"type": "composite", "buckets": []} if a is None else want_composite_page(world, COMPOSITE, b, a)
                      for b, a in zip(buckets, afters)]
            return dict(out, pages=[first, second], afters=afters, tuples=[len(b) for b in buckets])
        dead = [None if s.deleted is None else set(int(d) for d in np.nonzero(m.dead(i))[0]) for i, s in enumerate(segs)]
        return dict(out, cols=cols, masks=m.filter_masks(),
                    nodes={name: [term_buckets_ref.respond(body, cols, m.n_docs(), dead, m.filter_masks(), d, True) for d in docs]
                           for name, body in TERM_BUCKETS.items()})
    if kind == "request":
        cands = fscore_ref.all_candidates(oracle, segs, *Q)
        cols = fscore_ref.Columns(segs, {CANON["num"]: (m.num, np.dtype(np.int64))}, m.filters_by_id())
        r = compound_request(m, CANON)
        ms = request_ref.matched_sets(cands, segs, NQ, ("bool", r["clauses"]),
                                      request_ref.chains_of(NQ, fscore_functions(CANON)), cols)
        rows = request_ref.ordered(ms["rows"], SORT, sort_fields(m))
        page = request_ref.as_arrays(rows, K)
        return dict(page=page, matched=ms["matched"], sets=ms["rows"],
                    aggs=request_ref.agg_tables(REQUEST_AGGS, r["aggs"].nodes, agg_columns(m), m.filter_masks(), KEYS_OF, ms["rows"]),
                    collapse=request_ref.collapse_arrays(page, m.kw, dict(COLLAPSE, inner_sort=INNER_SORT), SORT, sort_fields(m)))
    if kind == "regex":
        world = X.World(m.keys)
        return [world.want(r) for r in regex_requests(m)]
    if kind == "suggest":
        world = SW.World(suggest_segments(m))
        return [world.want(r) for r in suggest_requests(m)]
    if kind == "highlight":
        hits = highlight_hits(m)
        return highlight_items(m, hits, highlight_specs(m, CANON["text"]))
    if kind == "highlight_batch":
        rows = oracle.search_batch(segs, *Q, K_PLAIN, strategy=oracle.BM25)
        doc, seg, _, count = rows
        hits = [[(int(seg[q, i]), int(doc[q, i])) for i in range(int(count[q]))] for q in range(len(count))]
        return dict(rows=rows, items=highlight_items(m, hits, highlight_specs(m, CANON["text"])))
    raise ValueError(kind)


def _expect(m, kind, oracle):
    if kind not in OLD_KINDS:
        return _expect_more(m, kind, oracle)
    Q = text_queries(m)
    segs = m.segs
    if kind == "plain":
        return oracle.search_batch(segs, *Q, K_PLAIN, strategy=oracle.BM25)
    if kind == "sorted":
        return expected_rows(all_hits(m, oracle), SORT, sort_fields(m))
    if kind == "cursor":
        rows, cursors = cursors_of(m, oracle)
        return dict(rows=rows, cursors=cursors)
    if kind == "bool":
        r = request(m, kind)
        return B.reference(oracle, segs, *Q, K, r["clauses"], q_filter=r["q_filter"], filters=m.filters_by_id())
    if kind == "tree":
        return booltree_ref.reference(oracle, segs, *Q, K, tree_descs(CANON), filters=alive_filters(m))
    if kind == "phrase":
        pq, cl, ph = phrase_queries(m)
        return P.reference(oracle, segs, *pq, K, ph, clauses=cl)
    if kind in ("fscore", "script"):
        cols = fscore_ref.Columns(segs, {CANON["num"]: (m.num, np.dtype(np.int64))}, m.filters_by_id())
        cands = fscore_ref.all_candidates(oracle, segs, *Q)
        if kind == "fscore":
            return fscore_ref.apply(cands, segs, fscore_functions(CANON), cols, K)[0]
        return script_ref.apply(cands, segs, [[("script", e)] for e in scripts(CANON)], cols, K)[0]
    if kind == "scan":
        qs, root = scan_queries(CANON)
        world = dict(n_docs=m.n_docs(), deleted=[None if s.deleted is None else m.dead(i) for i, s in enumerate(segs)],
                     filters=m.filters_by_id(), fields={CANON["num"]: m.num})
        assert not scan_ref.unsafe_docs(qs, world)
        rows, matched, _ = scan_ref.search(qs, world, K, root)
        return dict(rows=rows, matched=matched)
    if kind == "aggs":
        plan, cols = agg_plan(CANON), agg_columns(m)
        doc, seg, _, count = all_hits(m, oracle)
        docs = [[(int(seg[q, i]), int(doc[q, i])) for i in range(int(count[q]))] for q in range(len(count))]
        layout = V.ref_layout(plan.nodes, cols, KEYS_OF)
        tables = [V.dense(plan.nodes, layout, V.run(AGGS, cols, d), KEYS_OF) for d in docs]
        old_nodes = [nd for nd in plan.nodes if nd["body"]["type"] not in V.VALUE_TYPES]
        renum = {i: j for j, i in enumerate(i for i, nd in enumerate(plan.nodes) if nd in old_nodes)}
        flat = [dict(nd, parent=renum.get(nd["parent"], -1)) for nd in old_nodes]
        old_layout = agg_ref.ref_layout(flat, cols, KEYS_OF)
        old = [agg_ref.dense(flat, old_layout, agg_ref.run(V.strip(AGGS), cols, d), KEYS_OF) for d in docs]
        return dict(cols=cols, docs=docs, tables=tables, old=old, rows=oracle.search_batch(segs, *Q, K, strategy=oracle.BM25))
    if kind == "collapse":
        rows = CW.as_arrays(CW.sorted_rows(all_hits(m, oracle), None, sort_fields(m)), K)
        groups = collapse_ref.expected_arrays(*rows, m.kw, COLLAPSE["group_limit"], COLLAPSE["inner_from"],
                                              COLLAPSE["inner_size"], INNER_SORT, None, sort_fields(m))
        return dict(rows=rows, groups=groups)
    if kind == "rescore":
        return rescore_ref.reference(oracle, segs, *Q, K, rescore_spec(m))
    if kind == "expand":
        world = U.World(m.keys)
        return [world.want(r) for r in expand_requests(m)]
    if kind in ("vector", "hybrid"):
        r = request(m, kind)
        fields = m.vector_fields()
        if kind == "vector":
            live = lambda q, s, d: not m.dead(s)[d]
            return vector_reference(oracle, fields, [0, 0], r["clause_field"], r["qvecs"], r["alpha"], r["boost"],
                                    r["cand"], r["k_out"], live)
        return hybrid_ref.reference(oracle, segs, fields, r["clause_field"], *Q, K, r["qvecs"], r["alpha"], r["boost"],
                                    r["cand"], r["k_out"])
    if kind == "rerank":
        fields = rerank_fields(m)
        qs = rerank_queries(m)
        return dict(fields=fields, queries=qs,
                    rows=[oracle_rerank_segments(oracle, fields, q, "fields", K_OUT) for q in qs])
    raise ValueError(kind)


def vector_gaps(m, oracle):
    """the smallest score gap at a clause's cand boundary over the vector-only queries (its test orders rows only
    away from near-ties: the world keeps every state of every scenario away from them)"""
    r = request(m, "vector")
    live = lambda s, d: not m.dead(s)[d]
    return min(boundary_gap(oracle, m.vector_fields(), r["clause_field"], [r["qvecs"][q, :DIM], r["qvecs"][q, DIM:]],
                            r["boost"][q], r["cand"], live) for q in range(NV))


def hybrid_gaps(m, oracle):
    """the smallest gap hybrid_ref reports over the hybrid queries (tests/test_gpu_hybrid.py leaves a query below
    4e-5 out of its order check, and takes at most one in ten such: with 8 queries, none)"""
    return min(w["gap"] for w in expect(m, "hybrid", oracle))


# ---- what the device would be compared on, as plain data (equality of two expectations / two results) ------------
def digest(x):
    """any nesting of arrays, numbers, strings, dicts, lists, tuples, sets and slotted objects as hashable plain data;
    floats by their bit patterns"""
    if isinstance(x, np.ndarray):
        return ("nd", str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, (np.floating, float)):
        return ("f", np.float64(x).tobytes())
    if isinstance(x, (np.integer, np.bool_, int, bool, str, bytes, type(None))):
        return int(x) if isinstance(x, (np.integer, np.bool_)) else x
    if isinstance(x, dict):
        return ("d",) + tuple((digest(k), digest(v)) for k, v in sorted(x.items(), key=lambda kv: repr(kv[0])))
    if isinstance(x, (list, tuple)):
        return ("l",) + tuple(digest(v) for v in x)
    if isinstance(x, (set, frozenset)):
        return ("s",) + tuple(sorted(digest(v) for v in x))
    if hasattr(x, "__slots__"):
        return ("o",) + tuple(digest(getattr(x, n)) for n in x.__slots__)
    raise TypeError(type(x))


def checked_part(m, kind, want):
    """of an expectation, what the device check of the kind compares (rows up to k, counts, tables): two states whose
    checked parts are equal could not be told apart by the device test"""
    if kind == "sorted":
        return [(hits[:K], len(hits)) for hits in want]
    if kind == "cursor":
        out = []
        for hits, cur in zip(want["rows"], want["cursors"]):
            after = hits if cur is None else [h for h in hits if h.key > key_of(SORT, sort_fields(m), *cur)]
            out.append(([(h.seg, h.doc, h.score) for h in after[:PAGE + 1]], len(after)))
        return out
    if kind == "aggs":
        return dict(tables=want["tables"], old=want["old"], rows=want["rows"], matched=[len(d) for d in want["docs"]])
    if kind == "vector":
        return [(rows, total) for rows, total, _ in want]
    if kind == "hybrid":
        return [(w["rows"], w["total"]) for w in want]
    if kind == "rerank":
        return want["rows"]
    if kind == "date_aggs":
        return dict(want=want["want"], rows=want["rows"], matched=[len(d) for d in want["docs"]])
    if kind == "term_buckets":
        return dict(nodes={n: [term_buckets_ref.strip(r) for r in rs] for n, rs in want["nodes"].items()},
                    rows=want["rows"], matched=want["matched"])
    if kind == "request":
        return {n: v for n, v in want.items() if n != "sets"}
    return want


def hit_docs(m, kind, oracle=None):
    """the (segment, doc) pairs of the rows the kind's device check compares, in row order"""
    want = checked_part(m, kind, expect(m, kind, oracle))
    if kind in ("sorted", "cursor"):
        return [(int(h[0]), int(h[1])) for rows, _ in want for h in rows]
    if kind in ("vector", "hybrid"):
        return [(int(r[0]), int(r[1])) for rows, _ in want for r in rows]
    if kind == "aggs":
        return [sd for d in expect(m, kind, oracle)["docs"] for sd in d]
    rows = want["rows"] if isinstance(want, dict) else want
    doc, seg, count = rows[0], rows[1], rows[3]
    return [(int(seg[q, i]), int(doc[q, i])) for q in range(len(count)) for i in range(int(count[q]))]


def differs(m_a, m_b, kind, oracle=None):
    return digest(checked_part(m_a, kind, expect(m_a, kind, oracle))) != digest(checked_part(m_b, kind, expect(m_b, kind, oracle)))
