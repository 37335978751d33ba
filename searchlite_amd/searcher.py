"""Host mirror of the scorer interface, on top of the C ABI.

Names follow searchlite-core (query/wand.rs): `ScoredTerm`-style term lists, `execute_top_k`,
`RankedDoc`-style (doc_id, score) results, `QueryStats`.  GpuIndex owns an `slg_index`
(device-resident segments); PreparedBatch owns an `slg_batch`.

No CPU fallback lives here: every search goes through libsearchlite_gpu.so.
"""
from __future__ import annotations

import ctypes as C
import struct
import weakref
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from .segment import Segment, fold_terms, parse_query_terms, resolve_query

Bm25, Wand, Bmw = N.STRATEGY_BM25, N.STRATEGY_WAND, N.STRATEGY_BMW  # api/types.rs:6-13


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


def _f32(a, shape) -> Optional[np.ndarray]:
    """A contiguous f32 array of `shape` (a scalar or a row broadcasts); None stays None."""
    return None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float32), shape))


def device_count() -> int:
    n = N.load().slg_device_count()
    if n < 0:
        raise N.SlgError(n, N.last_error())
    return n


class GpuIndex:
    """All segments of one shard, staged in HBM (slg_index_create)."""

    def __init__(self, segments: Sequence[Segment], device: int = 0, tuning: Optional[dict] = None):
        """tuning: overrides of slg_tuning fields by name (e.g. {"pruning": 1}) on top of the
        defaults / SLG_* environment."""
        self._lib = N.load()
        self.segments = list(segments)
        self.device = device
        self._batches = weakref.WeakSet()  # closed with the index
        self._max_key_bytes = 0            # the longest key any set_terms() saw (suggest() sizes its text buffer by it)
        descs = (N.SegmentDesc * len(self.segments))()
        keep = []
        for i, s in enumerate(self.segments):
            descs[i] = self._desc(s, keep)
        tune = N.default_tuning()
        for name, val in (tuning or {}).items():
            if not hasattr(tune, name):
                raise KeyError(f"slg_tuning has no field {name!r}")
            setattr(tune, name, val)
        self._h = self._lib.slg_index_create_tuned(descs, len(self.segments), device, C.addressof(tune))
        if not self._h:
            raise N.SlgError(N.last_error_code() or N.ERR_INVALID, N.last_error())

    @staticmethod
    def _desc(s: Segment, keep: list) -> "N.SegmentDesc":
        nf = len(s.field_doc_len)
        ptrs = (C.c_void_p * nf)(*[_ptr(a) for a in s.field_doc_len])
        keep.append(ptrs)
        vec_rows = 0 if s.vec_values is None else int(s.vec_values.shape[0])
        return N.SegmentDesc(
            s.n_docs, s.n_terms, _ptr(s.term_offsets), _ptr(s.doc_ids), _ptr(s.tfs),
            _ptr(s.term_field), nf, C.addressof(ptrs), _ptr(s.field_avgdl),
            s.docs, s.k1, s.b, _ptr(s.deleted),
            s.vec_dim, s.vec_metric, _ptr(s.vec_offsets), _ptr(s.vec_values), vec_rows)

    # -- index updates (the reference's commit, api/writer.rs:106-240) ------------------------
    def update_deleted(self, seg: int, deleted: Optional[np.ndarray], live_docs: float) -> None:
        """New tombstones of segment `seg` (complete bitmap, bit d&7 of byte d>>3) and its new
        live_docs (slg_index_update_deleted); the mirrored Segment object follows."""
        bm = None if deleted is None else np.ascontiguousarray(deleted, dtype=np.uint8)
        N.check(self._lib.slg_index_update_deleted(self._h, seg, _ptr(bm), float(live_docs)))
        s = self.segments[seg]
        s.deleted = bm
        s.docs = float(live_docs)

    def add_segment(self, segment: Segment) -> int:
        """Stage one more segment at the next ordinal (slg_index_add_segment) -> the ordinal."""
        keep: list = []
        d = self._desc(segment, keep)
        ord_ = self._lib.slg_index_add_segment(self._h, C.addressof(d))
        if ord_ < 0:
            raise N.SlgError(ord_, N.last_error())
        self.segments.append(segment)
        return ord_

    def remove_segment(self, seg: int) -> None:
        N.check(self._lib.slg_index_remove_segment(self._h, seg))
        del self.segments[seg]

    def set_positions(self, seg: int, pos_offsets=None, positions=None) -> None:
        """The positions of segment `seg`'s postings (slg_index_set_positions): pos_offsets u64[P + 1] over the
        postings in the order of doc_ids / tfs, positions u32[pos_offsets[P]]; None, None removes them.  Phrase
        batches prepared afterwards see them; the mirrored Segment object follows."""
        po = None if pos_offsets is None else np.ascontiguousarray(pos_offsets, dtype=np.uint64)
        ps = None if positions is None else np.ascontiguousarray(positions, dtype=np.uint32)
        N.check(self._lib.slg_index_set_positions(self._h, seg, _ptr(po), _ptr(ps)))
        self.segments[seg].pos_offsets, self.segments[seg].positions = po, ps

    def set_terms(self, seg: int, keys: Sequence[str]) -> None:
        """The term dictionary of segment `seg` (slg_index_set_terms): keys[i] is the "field:term" key of term id
        i.  expand() needs one for every segment."""
        raw = [k.encode("utf-8") if isinstance(k, str) else bytes(k) for k in keys]
        offs = np.zeros(len(raw) + 1, dtype=np.uint32)
        np.cumsum([len(r) for r in raw], out=offs[1:])
        blob = np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)  # (one spare byte: never an empty array)
        N.check(self._lib.slg_index_set_terms(self._h, seg, _ptr(blob), _ptr(offs)))
        self._max_key_bytes = max(self._max_key_bytes, max((len(r) for r in raw), default=0))

    def set_terms_from_segments(self) -> None:
        """set_terms for every segment from its host dictionary (Segment.term_dict)."""
        for i, s in enumerate(self.segments):
            if s.term_dict is None:
                raise KeyError(f"segment {i} has no term dictionary")
            keys = [None] * s.n_terms
            for k, t in s.term_dict.items():
                keys[t] = k
            self.set_terms(i, keys)

    @classmethod
    def from_directory(cls, path: str, device: int = 0, tuning: Optional[dict] = None, **load) -> "GpuIndex":
        """The segments of a searchlite index directory (index_files.load_index(path, **load)), staged with their
        term dictionaries."""
        from .index_files import load_index
        ix = cls(load_index(path, **load).segments, device=device, tuning=tuning)
        try:
            ix.set_terms_from_segments()
        except Exception:
            ix.close()
            raise
        return ix

    def expand(self, requests) -> List[Tuple[np.ndarray, np.ndarray]]:
        """slg_expand_batch: requests = expand_request() dicts (or anything with their keys) -> per request
        (term_id_rows u32[n_keys, n_segs], distances u8[n_keys]), keys in the reference's order."""
        n = len(requests)
        reqs = (N.ExpandReq * max(n, 1))()
        keep = []
        for i, r in enumerate(requests):
            f = r["field"].encode("utf-8") if isinstance(r["field"], str) else bytes(r["field"])
            t = r["term"].encode("utf-8") if isinstance(r["term"], str) else bytes(r["term"])
            keep += [f, t]
            reqs[i] = N.ExpandReq(C.sizeof(N.ExpandReq), int(r["kind"]), f, t, len(f), len(t),
                                  int(r["max_expansions"]), int(r.get("max_edits", 0)),
                                  int(r.get("prefix_length", 0)), int(r.get("min_length", 0)))
        offs = np.zeros(n + 1, dtype=np.uint32)
        # the most keys the requests can yield: one call if that is a small array, else the size query first
        cap = max(sum(1 + r.max_expansions if r.kind == N.EXPAND_FUZZY else self.n_segs * r.max_expansions
                      for r in reqs[:n]), 1)
        if cap * self.n_segs > (1 << 24):
            N.check(self._lib.slg_expand_batch(self._h, reqs, n, _ptr(offs), 0, None, None))
            cap = max(int(offs[n]), 1)
        ids = np.zeros((cap, self.n_segs), dtype=np.uint32)
        dist = np.zeros(cap, dtype=np.uint8)
        N.check(self._lib.slg_expand_batch(self._h, reqs, n, _ptr(offs), cap, _ptr(ids), _ptr(dist)))
        return [(ids[int(offs[i]):int(offs[i + 1])].copy(), dist[int(offs[i]):int(offs[i + 1])].copy())
                for i in range(n)]

    def expand_phase_ms(self) -> Tuple[float, float]:
        """Diagnostic only (tools/expand_time.py): (device scan, host merge) of this thread's last expand(), in ms
        (slg_expand_phase_ms)."""
        a, b = C.c_double(0), C.c_double(0)
        N.check(self._lib.slg_expand_phase_ms(self._h, C.addressof(a), C.addressof(b)))
        return a.value, b.value

    def suggest(self, requests) -> List[List[Tuple[str, float, int]]]:
        """slg_suggest_batch: requests = suggest_request() dicts -> per request its options (text, score, doc_freq),
        best first, as the reference's completion suggester orders them; score is an np.float32."""
        n = len(requests)
        reqs = (N.SuggestReq * max(n, 1))()
        keep = []
        for i, r in enumerate(requests):
            f = r["field"].encode("utf-8") if isinstance(r["field"], str) else bytes(r["field"])
            t = r["term"].encode("utf-8") if isinstance(r["term"], str) else bytes(r["term"])
            keep += [f, t]
            fz = r.get("fuzzy")
            fo = dict(FUZZY_DEFAULTS, **fz) if fz is not None else dict(max_edits=0, prefix_length=0, max_expansions=0, min_length=0)
            reqs[i] = N.SuggestReq(C.sizeof(N.SuggestReq), f, t, len(f), len(t), int(r.get("size", 5)),
                                   0 if fz is None else 1, int(fo["max_edits"]), int(fo["prefix_length"]),
                                   int(fo["max_expansions"]), int(fo["min_length"]))
        offs = np.zeros(n + 2, dtype=np.uint32)
        # the most options the requests can yield, and their texts by the longest key any set_terms() saw; the size
        # query where that would be a large array
        cap = max(sum(min(r.size, N.MAX_SUGGEST_CANDIDATES) for r in reqs[:n]), 1)
        text_cap = max(cap * self._max_key_bytes, 1)
        if text_cap > (1 << 26):
            N.check(self._lib.slg_suggest_batch(self._h, reqs, n, _ptr(offs), 0, None, None, None, 0, None))
            cap, text_cap = max(int(offs[n]), 1), max(int(offs[n + 1]), 1)
        score = np.zeros(cap, dtype=np.float32)
        df = np.zeros(cap, dtype=np.uint64)
        toffs = np.zeros(cap + 1, dtype=np.uint32)
        text = np.zeros(text_cap, dtype=np.uint8)
        N.check(self._lib.slg_suggest_batch(self._h, reqs, n, _ptr(offs), cap, _ptr(score), _ptr(df), _ptr(toffs),
                                            text_cap, _ptr(text)))
        blob = text.tobytes()
        return [[(blob[int(toffs[i]):int(toffs[i + 1])].decode("utf-8"), score[i], int(df[i]))
                 for i in range(int(offs[r]), int(offs[r + 1]))] for r in range(n)]

    def suggest_phase_ms(self) -> Tuple[float, float]:
        """Diagnostic only (tools/suggest_time.py): (device part, host text copy) of this thread's last suggest(),
        in ms (slg_suggest_phase_ms)."""
        a, b = C.c_double(0), C.c_double(0)
        N.check(self._lib.slg_suggest_phase_ms(self._h, C.addressof(a), C.addressof(b)))
        return a.value, b.value

    def add_text_field(self, texts_per_segment) -> int:
        """slg_index_add_text_field: texts_per_segment[s] = the stored text of every doc of segment s (str or bytes;
        None or a value that is no string: an empty text), or None for a segment without the field -> the text
        field id highlight specs name."""
        assert len(texts_per_segment) == self.n_segs
        offs_p = (C.c_void_p * max(self.n_segs, 1))()
        bytes_p = (C.c_void_p * max(self.n_segs, 1))()
        keep = []
        for s, texts in enumerate(texts_per_segment):
            if texts is None:
                continue
            assert len(texts) == self.segments[s].n_docs
            raw = [t.encode("utf-8") if isinstance(t, str) else (bytes(t) if isinstance(t, (bytes, bytearray)) else b"")
                   for t in texts]
            offs = np.zeros(len(raw) + 1, dtype=np.uint64)
            np.cumsum([len(r) for r in raw], out=offs[1:])
            blob = np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)  # (one spare byte: never an empty array)
            keep += [offs, blob]
            offs_p[s], bytes_p[s] = offs.ctypes.data, blob.ctypes.data
        fid = self._lib.slg_index_add_text_field(self._h, offs_p, bytes_p)
        if fid < 0:
            raise N.SlgError(fid, N.last_error())
        return fid

    def remove_text_field(self, text_field: int) -> None:
        N.check(self._lib.slg_index_remove_text_field(self._h, int(text_field)))

    def highlight(self, hits, specs):
        """slg_highlight_batch: hits[q] = [(seg, doc), ...], specs[q] = [highlight_spec() / snippet_spec() dicts] ->
        result[q][hit][spec] = (status, [fragment bytes]) with the tags inserted (highlight.py)."""
        from .highlight import highlight_hits
        return highlight_hits(self._lib, self._h, hits, specs)

    def highlight_phase_ms(self) -> Tuple[float, float]:
        """Diagnostic only (tools/highlight_time.py): (count part, emit part) of this thread's last highlight call,
        in ms (slg_highlight_phase_ms)."""
        a, b = C.c_double(0), C.c_double(0)
        N.check(self._lib.slg_highlight_phase_ms(self._h, C.addressof(a), C.addressof(b)))
        return a.value, b.value

    def expanded_queries(self, queries: Sequence[str], default_field: str, fuzzy: Optional[dict] = None,
                         boost: float = 1.0):
        """The fuzzy expansion of a batch of query strings, folded into the arrays of a plain batch with plans.
        Every analysed term of a query is one source term and one plan leaf (summed); its expansions
        (expand(), FuzzyOptions `fuzzy`: max_edits 1, prefix_length 1, max_expansions 50, min_length 3 by default)
        weigh boost * the term's own boost * 1 / (distance + 1) in f32 (distance_weight, api/reader.rs:977-979) and go
        to its leaf; equal
        keys inside a query fold by summing and keep their first leaf (:2971-2983).  A query that folds to more
        than SLG_MAX_QUERY_TERMS terms raises SlgError(ERR_UNSUPPORTED).
        -> (q_offsets, q_terms[n, n_segs], q_weights, plans) with plans the q_leaf / q_plan / q_tie / q_nleaves
        keywords of search_plan()."""
        fz = dict(max_edits=1, prefix_length=1, max_expansions=50, min_length=3)
        fz.update(fuzzy or {})
        sources = []  # (query, "field:term", the term's own boost)
        for qi, q in enumerate(queries):
            sources += [(qi, key, tb) for key, tb in parse_query_terms(q, default_field)]
        reqs = [expand_request(N.EXPAND_FUZZY, key.split(":", 1)[0], key.split(":", 1)[1], **fz) for _, key, _ in sources]
        rows = self.expand(reqs) if reqs else []
        return fold_expansions(len(queries), [qi for qi, _, _ in sources], [key for _, key, _ in sources], rows,
                               self.n_segs, [np.float32(boost) * np.float32(tb) for _, _, tb in sources], queries)

    def search_fuzzy(self, queries: Sequence[str], default_field: str, k: int, fuzzy: Optional[dict] = None,
                     strategy: int = Wand, boost: float = 1.0):
        """A batch of query strings under SearchRequest.fuzzy: expanded_queries(), then the ordinary batch with
        plans -> (doc, seg, score, count)."""
        offs, terms, w, plans = self.expanded_queries(queries, default_field, fuzzy, boost)
        return self.search_plan(offs, terms, w, k, strategy=strategy, **plans)

    def search_patterns(self, nodes, k: int, strategy: int = Wand):
        """A batch of pattern nodes, one node one query: nodes = (kind, field, value, max_expansions, boost) with kind
        N.EXPAND_PREFIX (QueryNode::Prefix), N.EXPAND_WILDCARD (QueryNode::Wildcard) or N.EXPAND_REGEX
        (QueryNode::Regex).  expand(), then every key of a node at weight = boost on the node's one leaf
        (fold_expansions at distance 0), then the ordinary batch with plans -> (doc, seg, score, count).  A pattern
        the library refuses raises SlgError (ERR_UNSUPPORTED: the CPU path)."""
        nodes = list(nodes)
        for kind, *_ in nodes:
            if kind not in (N.EXPAND_PREFIX, N.EXPAND_WILDCARD, N.EXPAND_REGEX):
                raise ValueError(f"search_patterns: kind {kind} is not a prefix, wildcard or regex node")
        reqs = [expand_request(kind, field, value, mx) for kind, field, value, mx, _ in nodes]
        rows = self.expand(reqs) if reqs else []
        offs, terms, w, plans = fold_expansions(len(nodes), list(range(len(nodes))), [f"{f}:{v}" for _, f, v, _, _ in nodes],
                                                rows, self.n_segs, [np.float32(b) for *_, b in nodes] or 1.0,
                                                [v for _, _, v, _, _ in nodes])
        return self.search_plan(offs, terms, w, k, strategy=strategy, **plans)

    @property
    def generation(self) -> int:
        return int(self._lib.slg_index_generation(self._h))

    def tuning(self) -> "N.Tuning":
        t = N.Tuning()
        N.check(self._lib.slg_index_get_tuning(self._h, C.addressof(t)))
        return t

    # -- lifecycle -------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            for b in list(self._batches):  # batches die with their index
                b.close()
            self._lib.slg_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def n_segs(self) -> int:
        return len(self.segments)

    def info(self):
        ns, npost, nbytes = C.c_uint32(), C.c_uint64(), C.c_uint64()
        N.check(self._lib.slg_index_info(self._h, C.addressof(ns), C.addressof(npost),
                                         C.addressof(nbytes)))
        return {"n_segs": ns.value, "n_postings": npost.value, "device_bytes": nbytes.value}

    def champions(self, seg: int) -> np.ndarray:
        """The champion table of segment `seg` as the planner reads it (slg_index_fetch_champions):
        f32[n_terms, 68]; row[0..63] exact-rank lower bounds (row[0] the exact maximum), row[64..67] lower
        bounds of ranks 128, 256, 512 and 1024, over the live postings."""
        out = np.zeros((int(self.segments[seg].n_terms), 68), dtype=np.float32)
        N.check(self._lib.slg_index_fetch_champions(self._h, int(seg), out.ctypes.data))
        return out

    def trim_pool(self) -> int:
        """Give the pooled work buffers of finished batches back to the runtime -> bytes freed."""
        freed = C.c_uint64()
        N.check(self._lib.slg_index_trim_pool(self._h, C.addressof(freed)))
        return freed.value

    def set_stream(self, hip_stream) -> None:
        """Run on an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream; 0 is the
        HIP null stream = PyTorch's default stream).  None restores the index's own stream."""
        h = C.c_void_p(-1) if hip_stream is None else C.c_void_p(int(hip_stream) or None)
        N.check(self._lib.slg_index_set_stream(self._h, h))

    def profile(self, on: bool) -> None:
        N.check(self._lib.slg_profile_enable(self._h, int(on)))

    def profile_read(self) -> Tuple[int, float]:
        n, ms = C.c_uint32(), C.c_float()
        N.check(self._lib.slg_profile_read(self._h, C.addressof(n), C.addressof(ms)))
        return n.value, ms.value

    # -- doc filters (accept = !deleted && filter, api/reader.rs:3009-3018) ---------
    def add_filter(self, seg_masks) -> int:
        """Register a filter: seg_masks[s] = boolean array over the docs of segment s (True =
        passes) or None (all pass).  Returns the filter id queries refer to."""
        assert len(seg_masks) == self.n_segs
        packed = [None if m is None else np.packbits(np.asarray(m, dtype=bool), bitorder="little")
                  for m in seg_masks]
        ptrs = (C.c_void_p * self.n_segs)(*[None if b is None else b.ctypes.data for b in packed])
        rc = self._lib.slg_index_add_filter(self._h, ptrs)
        if rc < 0:
            N.check(rc)
        return rc

    def add_filter_range(self, seg_columns, lo, hi) -> int:
        """Filter built on the device from one numeric fast-field column per segment (int64 or
        float64 arrays of n_docs values): doc passes iff lo <= value <= hi."""
        assert len(seg_columns) == self.n_segs
        cols = [np.ascontiguousarray(c) for c in seg_columns]
        ptrs = (C.c_void_p * self.n_segs)(*[c.ctypes.data for c in cols])
        if all(c.dtype == np.int64 for c in cols):
            rc = self._lib.slg_index_add_filter_range_i64(self._h, ptrs, int(lo), int(hi))
        elif all(c.dtype == np.float64 for c in cols):
            rc = self._lib.slg_index_add_filter_range_f64(self._h, ptrs, float(lo), float(hi))
        else:
            raise TypeError("filter columns must all be int64 or all float64")
        if rc < 0:
            N.check(rc)
        return rc

    def add_filter_terms(self, term_ids, pass_if_absent: bool = True, and_masks=None) -> int:
        """Filter built on the device from resident posting lists (slg_index_add_filter_terms): the docs
        that hold none (pass_if_absent) / at least one of the terms; term_ids [n_terms, n_segs];
        and_masks: boolean masks per segment (or None) AND-ed with it."""
        tid = np.ascontiguousarray(term_ids, dtype=np.uint32).reshape(-1, self.n_segs)
        ptrs = None
        packed = None
        if and_masks is not None:
            assert len(and_masks) == self.n_segs
            packed = [None if m is None else np.packbits(np.asarray(m, dtype=bool), bitorder="little")
                      for m in and_masks]
            ptrs = (C.c_void_p * self.n_segs)(*[None if b is None else b.ctypes.data for b in packed])
        rc = self._lib.slg_index_add_filter_terms(self._h, tid.ctypes.data if tid.size else None, tid.shape[0],
                                                  int(bool(pass_if_absent)), ptrs)
        if rc < 0:
            N.check(rc)
        return rc

    def remove_filter(self, filter_id: int) -> None:
        N.check(self._lib.slg_index_remove_filter(self._h, filter_id))

    def add_filter_trees(self, trees) -> List[int]:
        """Filters built on the device from filter trees over the registered agg fields, all in one update of
        the index (slg_index_add_filter_trees).  trees: filters.FilterProgram objects (filters.compile_filter) or
        (nodes, ords) pairs, nodes being dicts of slg_filter_node fields in postfix order.  -> the filter ids,
        one per tree; on an error none is registered."""
        from .filters import tree_array
        trees = list(trees)
        arr, keep = tree_array(trees)
        ids = np.full(max(len(trees), 1), -1, dtype=np.int32)
        N.check(self._lib.slg_index_add_filter_trees(self._h, arr, len(trees), ids.ctypes.data))
        del keep
        return [int(i) for i in ids[:len(trees)]]

    def fetch_filter(self, filter_id: int) -> List[np.ndarray]:
        """The docs that are alive and pass a registered filter of any kind (slg_index_fetch_filter): one
        boolean array per segment."""
        out = []
        for s, seg in enumerate(self.segments):
            n = int(seg.n_docs)
            buf = np.zeros(max((n + 7) // 8, 1), dtype=np.uint8)
            N.check(self._lib.slg_index_fetch_filter(self._h, int(filter_id), s, buf.ctypes.data))
            out.append(np.unpackbits(buf, bitorder="little")[:n].astype(bool))
        return out

    # -- nested filters (query/filters.rs:13-188: same-object matching over arrays of objects) ----
    def _u32_ptrs(self, arrays, keep):
        """arrays[s]: an array or None -> a pointer array over contiguous u32 copies (kept alive in keep)."""
        ptrs = []
        for a in arrays:
            if a is None:
                ptrs.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=np.uint32)
            if a.size == 0:
                a = np.zeros(1, np.uint32)
            keep.append(a)
            ptrs.append(a.ctypes.data)
        return (C.c_void_p * self.n_segs)(*ptrs)

    def add_nested_path(self, per_segment, parent: int = -1) -> int:
        """Register a nested path (slg_index_add_nested_path).  per_segment[s]: None (no doc of the segment has an
        object), the objects per doc (u32[n_docs]), or (counts, (parent_offsets u32[n_docs + 1], parents)) with the
        parent lists of the reference's _nested_parent column (None: nothing binds).  parent: the id of the path
        one level up, or -1.  Returns the path id (ids are never reused)."""
        assert len(per_segment) == self.n_segs
        counts, poffs, pvals = [], [], []
        for s, v in enumerate(per_segment):
            c, par = (v if isinstance(v, tuple) else (v, None))
            if c is not None:
                assert len(c) == int(self.segments[s].n_docs), "one count per doc"
            if par is not None:
                assert len(par[0]) == int(self.segments[s].n_docs) + 1, "one parent offset per doc + 1"
            counts.append(c)
            poffs.append(None if par is None else par[0])
            pvals.append(None if par is None else par[1])
        keep: list = []
        rc = self._lib.slg_index_add_nested_path(self._h, int(parent), self._u32_ptrs(counts, keep),
                                                 self._u32_ptrs(poffs, keep), self._u32_ptrs(pvals, keep))
        if rc < 0:
            N.check(rc)
        return rc

    def remove_nested_path(self, path_id: int) -> None:
        """Unregister a nested path and the nested fields under it (slg_index_remove_nested_path)."""
        N.check(self._lib.slg_index_remove_nested_path(self._h, int(path_id)))

    def _add_nested_column(self, path_id, per_segment, dt, n_ords=None) -> int:
        assert len(per_segment) == self.n_segs
        keep: list = []
        for s, v in enumerate(per_segment):
            if v is not None:
                assert len(v[0]) == int(self.segments[s].n_docs) + 1, "one doc offset per doc + 1"
        po = self._u32_ptrs([None if v is None else v[0] for v in per_segment], keep)
        pj = self._u32_ptrs([None if v is None else v[1] for v in per_segment], keep)
        vals = []
        for v in per_segment:
            a = None if v is None else np.ascontiguousarray(v[2], dtype=dt)
            if a is not None and a.size == 0:
                a = np.zeros(1, dt)
            keep.append(a)
            vals.append(None if a is None else a.ctypes.data)
        pv = (C.c_void_p * self.n_segs)(*vals)
        if n_ords is not None:
            rc = self._lib.slg_index_add_nested_field_ord(self._h, int(path_id), po, pj, pv, int(n_ords))
        elif dt == np.int64:
            rc = self._lib.slg_index_add_nested_field_i64(self._h, int(path_id), po, pj, pv)
        else:
            rc = self._lib.slg_index_add_nested_field_f64(self._h, int(path_id), po, pj, pv)
        if rc < 0:
            N.check(rc)
        return rc

    def add_nested_field(self, path_id: int, per_segment, dtype) -> int:
        """Register a numeric nested value column under a path (slg_index_add_nested_field_i64 / _f64).
        per_segment[s]: None (the segment has no value) or (doc_offsets u32[n_docs + 1], object_offsets, values),
        the arrays of the reference's I64Nested / F64Nested column.  int64 values stay int64 on the device.
        Returns the nested field id (ids are never reused)."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.int64), np.dtype(np.float64)):
            raise TypeError("numeric nested fields are int64 or float64")
        return self._add_nested_column(path_id, per_segment, dt)

    def add_nested_keyword_field(self, path_id: int, per_segment_ords, n_ords: int) -> int:
        """Register a keyword nested column (slg_index_add_nested_field_ord): per_segment_ords as add_nested_field's
        with ordinals into ONE dictionary of n_ords keys, the caller's."""
        return self._add_nested_column(path_id, per_segment_ords, np.dtype(np.uint32), n_ords)

    def remove_nested_field(self, nested_field_id: int) -> None:
        N.check(self._lib.slg_index_remove_nested_field(self._h, int(nested_field_id)))

    def add_nested_filter_trees(self, trees) -> List[int]:
        """Filters built on the device from filter trees with Nested nodes, all in one update of the index
        (slg_index_add_nested_filter_trees).  trees: filters.NestedFilterProgram objects
        (filters.compile_nested_filter) or (scopes, nodes, ords) triples.  -> the filter ids, one per tree; on an
        error none is registered."""
        from .filters import nested_tree_array
        trees = list(trees)
        arr, keep = nested_tree_array(trees)
        ids = np.full(max(len(trees), 1), -1, dtype=np.int32)
        N.check(self._lib.slg_index_add_nested_filter_trees(self._h, arr, len(trees), ids.ctypes.data))
        del keep
        return [int(i) for i in ids[:len(trees)]]

    # -- sort fields (query/sort.rs: `sort` on numeric fast fields) -----------------------------
    def add_sort_field(self, per_segment_values, dtype) -> int:
        """Register a numeric fast field for field-sorted search (slg_index_add_sort_field_i64 / _f64).
        per_segment_values[s]: the values of segment s's docs, either a list of n_docs arrays (empty = Missing)
        or a CSR pair (offsets[n_docs + 1], values), or None (every doc Missing).  dtype: np.int64 or
        np.float64.  Returns the sort field id (ids are never reused)."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.int64), np.dtype(np.float64)):
            raise TypeError("sort fields are int64 or float64")
        assert len(per_segment_values) == self.n_segs
        keep = []
        offs_p, vals_p = [], []
        for s, v in enumerate(per_segment_values):
            if v is None:
                offs_p.append(None)
                vals_p.append(None)
                continue
            if isinstance(v, tuple):
                offs = np.ascontiguousarray(v[0], dtype=np.uint32)
                vals = np.ascontiguousarray(v[1], dtype=dt)
            else:
                lens = np.array([len(x) for x in v], dtype=np.uint64)
                offs = np.zeros(len(v) + 1, dtype=np.uint32)
                offs[1:] = np.cumsum(lens)
                vals = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=dt) for x in v]) if len(v) else
                                            np.zeros(0, dt), dtype=dt)
            assert len(offs) == int(self.segments[s].n_docs) + 1, "one offset per doc + 1"
            if vals.size == 0:
                vals = np.zeros(1, dt)
            keep += [offs, vals]
            offs_p.append(offs.ctypes.data)
            vals_p.append(vals.ctypes.data)
        po = (C.c_void_p * self.n_segs)(*offs_p)
        pv = (C.c_void_p * self.n_segs)(*vals_p)
        fn = self._lib.slg_index_add_sort_field_i64 if dt == np.int64 else self._lib.slg_index_add_sort_field_f64
        rc = fn(self._h, po, pv)
        if rc < 0:
            N.check(rc)
        return rc

    def remove_sort_field(self, sort_field_id: int) -> None:
        N.check(self._lib.slg_index_remove_sort_field(self._h, sort_field_id))

    # -- aggregation fields (query/aggs/mod.rs; lifecycle and ids as sort fields) ----------------
    def _csr_ptrs(self, per_segment, dt, keep):
        """per_segment[s]: a list of n_docs arrays, a CSR pair (offsets[n_docs + 1], values) or None ->
        the two pointer arrays of slg_index_add_*_field_*."""
        assert len(per_segment) == self.n_segs
        offs_p, vals_p = [], []
        for s, v in enumerate(per_segment):
            if v is None:
                offs_p.append(None)
                vals_p.append(None)
                continue
            if isinstance(v, tuple):
                offs = np.ascontiguousarray(v[0], dtype=np.uint32)
                vals = np.ascontiguousarray(v[1], dtype=dt)
            else:
                offs = np.zeros(len(v) + 1, dtype=np.uint32)
                offs[1:] = np.cumsum(np.array([len(x) for x in v], dtype=np.uint64))
                vals = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=dt) for x in v]) if len(v) else
                                            np.zeros(0, dt), dtype=dt)
            assert len(offs) == int(self.segments[s].n_docs) + 1, "one offset per doc + 1"
            if vals.size == 0:
                vals = np.zeros(1, dt)
            keep += [offs, vals]
            offs_p.append(offs.ctypes.data)
            vals_p.append(vals.ctypes.data)
        return (C.c_void_p * self.n_segs)(*offs_p), (C.c_void_p * self.n_segs)(*vals_p)

    def add_agg_field(self, per_segment, dtype) -> int:
        """Register a numeric column for aggregations (slg_index_add_agg_field_i64 / _f64); per_segment as
        add_sort_field.  Returns the agg field id (ids are never reused)."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.int64), np.dtype(np.float64)):
            raise TypeError("numeric agg fields are int64 or float64")
        keep: list = []
        po, pv = self._csr_ptrs(per_segment, dt, keep)
        fn = self._lib.slg_index_add_agg_field_i64 if dt == np.int64 else self._lib.slg_index_add_agg_field_f64
        rc = fn(self._h, po, pv)
        if rc < 0:
            N.check(rc)
        return rc

    def add_agg_keyword_field(self, per_segment_ords, n_ords: int) -> int:
        """Register a keyword column (slg_index_add_agg_field_ord): per segment the docs' ordinals into ONE
        dictionary of n_ords keys, the caller's."""
        keep: list = []
        po, pv = self._csr_ptrs(per_segment_ords, np.dtype(np.uint32), keep)
        rc = self._lib.slg_index_add_agg_field_ord(self._h, po, pv, int(n_ords))
        if rc < 0:
            N.check(rc)
        return rc

    def remove_agg_field(self, agg_field_id: int) -> None:
        N.check(self._lib.slg_index_remove_agg_field(self._h, agg_field_id))

    def rank_agg_field(self, agg_field_id: int) -> int:
        """Build the value ranks of a registered column (slg_index_rank_agg_field), what cardinality and percentiles
        nodes need of a numeric field.  Returns the number of distinct values (n_ords for a keyword field); a
        second call only returns it."""
        rc = int(self._lib.slg_index_rank_agg_field(self._h, agg_field_id))
        if rc < 0:
            N.check(rc)
        return rc

    def search_aggs(self, q_offsets, q_terms, q_weights, k: int, aggs, sort=None, strategy: int = Wand,
                    q_filter=None, **plans):
        """Batch search with aggregations (slg_batch_prepare_aggs).  aggs: an N.AggSpec or an aggs.AggPlan;
        sort: None = score order, else as search_sorted.
        -> (doc, seg, score, count, matched, tables, layout): tables[i] [nq, parent_rows, rows] of node i
        (PreparedBatch.aggs), layout as PreparedBatch.agg_layout."""
        b = self.prepare(q_offsets, q_terms, q_weights, k, strategy, q_filter, sort=sort, aggs=aggs, **plans)
        try:
            b.run()
            return b.fetch() + (b.matched_counts(), b.aggs(), b.agg_layout())
        finally:
            b.close()

    def search_top_hits(self, q_offsets, q_terms, q_weights, k: int, aggs, sort=None, strategy: int = Wand,
                        q_filter=None, top_hits=None, **plans):
        """Batch search with top_hits aggregations (slg_batch_prepare_top_hits).  aggs: an aggs.AggPlan with
        top_hits nodes, or an N.AggSpec / None with top_hits an N.TopHitsSpec; sort: None = score order.
        -> (doc, seg, score, count, matched, tables, layout, hits): as search_aggs (tables and layout empty
        without an aggregation node), and the dict of PreparedBatch.top_hits.  A child of a terms, histogram, range
        or date_histogram aggregation costs 8 bytes x max_entries of run scratch per query, 4 MB at the default: set
        it through aggs.agg_spec(..., top_hits_max_entries=n) or N.TopHitsSpec.max_entries.  `fields` and `snippet` of the
        reference's hits are doc-store work and stay with the caller."""
        b = self.prepare(q_offsets, q_terms, q_weights, k, strategy, q_filter, sort=sort, aggs=aggs,
                         top_hits=top_hits, **plans)
        try:
            b.run()
            has = b.agg_spec is not None
            return b.fetch() + (b.matched_counts(), b.aggs() if has else [], b.agg_layout() if has else [],
                                b.top_hits())
        finally:
            b.close()

    def search_rescore(self, q_offsets, q_terms, q_weights, k: int, rescore, strategy: int = Wand, q_filter=None,
                       **plans):
        """Batch search with a query rescore (slg_batch_prepare_rescore).  rescore: a dict with q_offsets, q_terms
        ([total, n_segs]), q_weights, window (a number or one per query) and optionally mode (RESCORE_*, a number
        or one per query), q_leaf, q_plan, q_tie, q_nleaves, q_min_match; **plans: the first pass's score plan
        arrays of prepare().  -> (doc, seg, score, count, first_score, rescore_score, rescored)."""
        b = self.prepare(q_offsets, q_terms, q_weights, k, strategy, q_filter, rescore=rescore, **plans)
        try:
            b.run()
            return b.fetch() + b.rescore_details()
        finally:
            b.close()

    def search_batch_bool(self, q_offsets, q_terms, q_weights, k: int, clauses, sort=None, strategy: int = Wand,
                          q_filter=None, want_stats: bool = False, **plans):
        """Batch search with boolean clauses (slg_batch_prepare_bool).  clauses: a dict with c_offsets [nq + 1],
        c_terms ([total, n_segs]), c_group [total], g_offsets [nq + 1], g_kind (BOOL_MUST / _SHOULD / _MUST_NOT per
        group) and optionally q_min_should (a number or one per query); sort: None = score order, else as
        search_sorted; **plans: the score plan arrays of prepare().
        -> (doc, seg, score, count[, stats]) in score order, (doc, seg, score, count[, stats], matched) sorted."""
        b = self.prepare(q_offsets, q_terms, q_weights, k, strategy, q_filter, sort=sort, clauses=clauses, **plans)
        try:
            b.run()
            return b.fetch(want_stats) + ((b.matched_counts(),) if sort is not None else ())
        finally:
            b.close()

    def search_batch_bool_tree(self, q_offsets, q_terms, q_weights, k: int, clause_tree, sort=None,
                               strategy: int = Wand, q_filter=None, want_stats: bool = False, **plans):
        """Batch search with a nested boolean matcher per query (slg_batch_prepare_bool_tree).  clause_tree: the dict
        of booltree.compile_matchers (term groups, filter leaves and a post-order node table per query); sort: None =
        score order, else as search_sorted; **plans: the score plan arrays of prepare().
        Returns what search_batch_bool returns."""
        b = self.prepare(q_offsets, q_terms, q_weights, k, strategy, q_filter, sort=sort, clause_tree=clause_tree,
                         **plans)
        try:
            b.run()
            return b.fetch(want_stats) + ((b.matched_counts(),) if sort is not None else ())
        finally:
            b.close()

    def search_batch_phrase(self, q_offsets, q_terms, q_weights, k: int, phrases, clauses=None, sort=None,
                            strategy: int = Wand, q_filter=None, want_stats: bool = False, **plans):
        """Batch search with phrase groups (slg_batch_prepare_phrase).  phrases: a dict with p_offsets [nq + 1],
        p_kind (BOOL_MUST / _SHOULD / _MUST_NOT per phrase), p_slop, v_offsets [n_phrases + 1], t_offsets
        [n_variants + 1], t_terms ([total, n_segs]) and optionally q_min_should (a number or one per query, over
        term and phrase groups); clauses: the term groups, the dict of search_batch_bool without q_min_should, or
        None; the segments' positions: set_positions.  Returns what search_batch_bool returns."""
        b = self.prepare(q_offsets, q_terms, q_weights, k, strategy, q_filter, sort=sort, clauses=clauses,
                         phrases=phrases, **plans)
        try:
            b.run()
            return b.fetch(want_stats) + ((b.matched_counts(),) if sort is not None else ())
        finally:
            b.close()

    def search_batch_fscore(self, q_offsets, q_terms, q_weights, k: int, functions, sort=None, strategy: int = Wand,
                            q_filter=None, want_stats: bool = False, **plans):
        """Batch search under a function_score per query (slg_batch_prepare_fscore).  functions: the list of
        fscore_spec(), one entry per query (None: the query is left as it is); columns are agg field ids
        (add_agg_field), function filters are filter ids (add_filter*); sort: None = order of the new score, else
        as search_sorted; **plans: the score plan arrays of prepare().
        -> (doc, seg, score, count[, stats]) in score order, (doc, seg, score, count[, stats], matched) sorted."""
        b = self.prepare(q_offsets, q_terms, q_weights, k, strategy, q_filter, sort=sort, fscore=functions, **plans)
        try:
            b.run()
            return b.fetch(want_stats) + ((b.matched_counts(),) if sort is not None else ())
        finally:
            b.close()

    def search_batch_script(self, q_offsets, q_terms, q_weights, k: int, scripts, fscore=None, script_order="outer",
                            sort=None, strategy: int = Wand, q_filter=None, want_stats: bool = False, **plans):
        """Batch search under a script_score per query (slg_batch_prepare_script).  scripts: the list of
        script.script_spec(), one entry per query (None: the query is left as it is); fields are agg field ids
        (add_agg_field); fscore: a function_score stage beside it (the list of fscore_spec()), script_order "outer"
        = script_score{query: function_score}, "inner" = function_score{query: script_score}; sort: None = order
        of the new score, else as search_sorted; **plans: the score plan arrays of prepare().
        -> (doc, seg, score, count[, stats]) in score order, (doc, seg, score, count[, stats], matched) sorted."""
        b = self.prepare(q_offsets, q_terms, q_weights, k, strategy, q_filter, sort=sort, fscore=fscore, script=scripts,
                         script_order=script_order, **plans)
        try:
            b.run()
            return b.fetch(want_stats) + ((b.matched_counts(),) if sort is not None else ())
        finally:
            b.close()

    def prepare_scan(self, queries, k: int, sort=None, aggs=None, q_filter=None) -> "ScanBatch":
        """A batch of unscored root queries (slg_batch_prepare_scan).  queries: one dictionary per query, as
        scan.scan_spec takes them (match_all, constant_score, rank_feature), or its (spec, keep) pair; sort: None =
        score order, else as search_sorted; aggs: an N.AggSpec or an aggs.AggPlan, or None; q_filter: the root
        filter id per query, or None; k may be 0."""
        return ScanBatch(self, queries, k, sort=sort, aggs=aggs, q_filter=q_filter)

    def search_scan(self, queries, k: int, sort=None, aggs=None, q_filter=None, want_stats: bool = False):
        """prepare_scan, one run and the results: -> (doc, seg, score, count[, stats], matched), and with aggs also
        (tables, layout) as search_aggs returns them.  matched is total_matches, in every order and for k = 0."""
        b = self.prepare_scan(queries, k, sort=sort, aggs=aggs, q_filter=q_filter)
        try:
            b.run()
            out = b.fetch(want_stats) + (b.matched_counts(),)
            return out + ((b.aggs(), b.agg_layout()) if aggs is not None else ())
        finally:
            b.close()

    def search_sorted(self, q_offsets, q_terms, q_weights, k: int, sort, strategy: int = Wand, q_filter=None,
                      **plans):
        """Field-sorted batch search (slg_batch_prepare_sorted).  sort: [(field, order)], field = a sort field id
        or "_score", order = "asc" / "desc"; **plans: the score plan arrays of prepare().
        -> (doc, seg, score, count, matched)."""
        b = self.prepare(q_offsets, q_terms, q_weights, k, strategy, q_filter, sort=sort, **plans)
        try:
            b.run()
            return b.fetch() + (b.matched_counts(),)
        finally:
            b.close()

    def search_after(self, q_offsets, q_terms, q_weights, k: int, cursors, sort=None, strategy: int = Wand,
                     q_filter=None, **plans):
        """The next page (slg_batch_prepare_after): per query the top k strictly after its cursor.  cursors: one
        per query, None (a first page) or (values, segment_ord, doc_id) with values one per sort part (score
        order: (score,)) — an int for an i64 field, a float for an f64 field or a score, None for Missing; or
        an N.SortCursor.  sort: None = score order, else as search_sorted.
        -> (doc, seg, score, count, matched, seen)."""
        b = self.prepare(q_offsets, q_terms, q_weights, k, strategy, q_filter, sort=sort, cursors=cursors, **plans)
        try:
            b.run()
            return b.fetch() + (b.matched_counts(), b.cursor_seen())
        finally:
            b.close()

    # -- search ----------------------------------------------------------------------
    def prepare(self, q_offsets, q_terms, q_weights, k: int, strategy: int = Wand,
                q_filter=None, q_leaf=None, q_plan=None, q_tie=None, q_nleaves=None,
                q_leaf_offsets=None, leaf_group=None, q_group_offsets=None, group_plan=None,
                group_tie=None, q_node_offsets=None, node_kind=None, node_tie=None, node_parent=None,
                q_min_match=None, sort=None, cursors=None, hybrid=False, aggs=None,
                rescore=None, clauses=None, phrases=None, fscore=None, collapse=None,
                clause_tree=None, script=None, script_order="outer", top_hits=None,
                composite=None, term_buckets=None) -> "PreparedBatch":
        """q_leaf / q_plan / q_tie / q_nleaves: score plans; leaf_group / group_plan / group_tie with
        their per-query offsets: two-level plans; q_node_offsets / node_kind / node_tie / node_parent:
        trees of any shape, node by node in pre-order (slg_batch_prepare_plans, slg_score_plans);
        q_min_match: minimum_should_match per query (leaves that must hold a doc); sort: a field sort
        (search_sorted) -> slg_batch_prepare_sorted; cursors: a cursor per query (search_after) ->
        slg_batch_prepare_after; hybrid: the text side of a hybrid text + vector search ->
        slg_batch_prepare_hybrid (PreparedBatch.hybrid_device); aggs: an N.AggSpec or aggs.AggPlan ->
        slg_batch_prepare_aggs (PreparedBatch.aggs); rescore: the dict of search_rescore ->
        slg_batch_prepare_rescore (PreparedBatch.rescore_details); clauses: the dict of search_batch_bool ->
        slg_batch_prepare_bool (score order, or with sort); phrases: the dict of search_batch_phrase ->
        slg_batch_prepare_phrase (with clauses as its term groups, or without); fscore: one function_score per
        query, the list of fscore_spec() (or its result) -> slg_batch_prepare_fscore (score order, or with sort);
        collapse: the dict of search_collapse -> slg_batch_prepare_collapse (score order, with sort and / or cursors;
        PreparedBatch.collapse_groups); clause_tree: the dict of search_batch_bool_tree ->
        slg_batch_prepare_bool_tree (score order, or with sort); script: one script_score per query, the list of
        script.script_spec() (or its result) -> slg_batch_prepare_script (score order, or with sort), alone or with
        fscore as its second stage: script_order "outer" is script_score{query: function_score}, "inner" is
        function_score{query: script_score}; top_hits: an N.TopHitsSpec (an aggs.AggPlan passed as aggs brings its
        own) -> slg_batch_prepare_top_hits (score order or with sort, with aggs or without;
        PreparedBatch.top_hits); composite: an N.CompositeSpec (an aggs.AggPlan passed as aggs brings its own) ->
        slg_batch_prepare_composite (score order or with sort, with aggs or without; PreparedBatch.composite);
        term_buckets: an N.TermBucketSpec (an aggs.AggPlan passed as aggs brings its own) ->
        slg_batch_prepare_term_buckets (score order or with sort, with aggs or without; PreparedBatch.term_buckets)."""
        return PreparedBatch(self, q_offsets, q_terms, q_weights, k, strategy, q_filter,
                             q_leaf, q_plan, q_tie, q_nleaves, q_leaf_offsets, leaf_group,
                             q_group_offsets, group_plan, group_tie, q_node_offsets, node_kind, node_tie, node_parent,
                             q_min_match, sort, cursors, hybrid, aggs, rescore, clauses, phrases, fscore, collapse,
                             clause_tree, script, script_order, top_hits, composite, term_buckets)

    def prepare_request(self, q_offsets, q_terms, q_weights, k: int, strategy: int = Wand, q_filter=None,
                        **kinds) -> "PreparedBatch":
        """A compound request (slg_batch_prepare_request): several batch kinds in one batch.  **kinds: the keyword
        arguments of prepare() — sort, cursors, clauses, phrases, clause_tree, fscore, script, script_order, aggs,
        top_hits, composite, term_buckets, rescore, collapse and the score plan arrays — every one that is given
        is asked for, and the library refuses the combinations that are not built (ERR_UNSUPPORTED, the message
        naming the pair).  The batch has the fetch methods of every kind asked for: fetch, matched_counts,
        cursor_seen, aggs, top_hits, composite, term_buckets, rescore_details, collapse_groups, highlight."""
        if "hybrid" in kinds or "request" in kinds:
            raise N.SlgError(N.ERR_UNSUPPORTED, "prepare_request takes no `hybrid` or `request` argument (a hybrid batch "
                                                "keeps its own entry point: prepare(hybrid=True))")
        return PreparedBatch(self, q_offsets, q_terms, q_weights, k, strategy, q_filter, request=True, **kinds)

    def search_request(self, q_offsets, q_terms, q_weights, k: int, strategy: int = Wand, q_filter=None,
                       want_stats: bool = False, **kinds) -> dict:
        """prepare_request, one run and everything the request asked for, as a dict: doc, seg, score, count[, stats];
        matched (a sort, a cursor or a collector); seen (cursors); aggs and agg_layout; top_hits; composite;
        term_buckets; rescore (first_score, rescore_score, rescored); collapse."""
        b = self.prepare_request(q_offsets, q_terms, q_weights, k, strategy, q_filter, **kinds)
        try:
            b.run()
            out = dict(zip(("doc", "seg", "score", "count", "stats"), b.fetch(want_stats)))
            collectors = [x is not None for x in (b.agg_spec, b.top_hits_spec, b.composite_spec, b.term_bucket_spec)]
            if b.sorted or b.after or any(collectors):
                out["matched"] = b.matched_counts()
            if b.after:
                out["seen"] = b.cursor_seen()
            if collectors[0]:
                out["aggs"], out["agg_layout"] = b.aggs(), b.agg_layout()
            if collectors[1]:
                out["top_hits"] = b.top_hits()
            if collectors[2]:
                out["composite"] = b.composite()
            if collectors[3]:
                out["term_buckets"] = b.term_buckets()
            if b.is_rescore:
                out["rescore"] = b.rescore_details()
            if b.is_collapse:
                out["collapse"] = b.collapse_groups()
            return out
        finally:
            b.close()

    def search_term_buckets(self, q_offsets, q_terms, q_weights, k: int, aggs, sort=None, strategy: int = Wand,
                            q_filter=None, term_buckets=None, **plans):
        """Batch search with significant_terms / rare_terms aggregations (slg_batch_prepare_term_buckets).  aggs: an
        aggs.AggPlan with such nodes, or an N.AggSpec / None with term_buckets an N.TermBucketSpec.
        -> (doc, seg, score, count, matched, tables, layout, buckets): as search_aggs (tables and layout empty
        without an aggregation node), and the dict of PreparedBatch.term_buckets."""
        b = self.prepare(q_offsets, q_terms, q_weights, k, strategy, q_filter, sort=sort, aggs=aggs,
                         term_buckets=term_buckets, **plans)
        try:
            b.run()
            has = b.agg_spec is not None
            return b.fetch() + (b.matched_counts(), b.aggs() if has else [], b.agg_layout() if has else [],
                                b.term_buckets())
        finally:
            b.close()

    def prepare_composite(self, q_offsets, q_terms, q_weights, k: int, aggs, sort=None, strategy: int = Wand,
                          q_filter=None, composite=None, **plans) -> "PreparedBatch":
        """A batch with a composite aggregation (slg_batch_prepare_composite).  aggs: an aggs.AggPlan with a
        composite, or an N.AggSpec / None with composite an N.CompositeSpec.  One prepared batch pages through a
        bucket set: set_composite_after(bounds), run(), composite(), again."""
        return self.prepare(q_offsets, q_terms, q_weights, k, strategy, q_filter, sort=sort, aggs=aggs,
                            composite=composite, **plans)

    def search_composite(self, q_offsets, q_terms, q_weights, k: int, aggs, sort=None, strategy: int = Wand,
                         q_filter=None, composite=None, lower=None, **plans):
        """Batch search with a composite aggregation: one page.  lower: per query the inclusive packed lower bound
        (aggs.composite_lower_bound), None = the first page.
        -> (doc, seg, score, count, matched, tables, layout, page): as search_aggs (tables and layout empty
        without an aggregation node), and the dict of PreparedBatch.composite."""
        b = self.prepare_composite(q_offsets, q_terms, q_weights, k, aggs, sort, strategy, q_filter, composite, **plans)
        try:
            if lower is not None:
                b.set_composite_after(lower)
            b.run()
            has = b.agg_spec is not None
            return b.fetch() + (b.matched_counts(), b.aggs() if has else [], b.agg_layout() if has else [],
                                b.composite())
        finally:
            b.close()

    def search_collapse(self, q_offsets, q_terms, q_weights, k: int, collapse, sort=None, cursors=None,
                        strategy: int = Wand, q_filter=None, **plans):
        """Batch search with field collapsing (slg_batch_prepare_collapse).  collapse: a dict with field (the id of
        a keyword column, add_agg_keyword_field), group_limit (the request's limit) and optionally inner_from (0),
        inner_size (0: no inner hits) and inner_sort (None: the batch's own order, else as search_sorted's sort;
        [] is `_score` desc); sort / cursors as search_sorted / search_after; k = candidate_size + 1.
        -> (doc, seg, score, count, groups): the rows, and the dict of PreparedBatch.collapse_groups."""
        b = self.prepare(q_offsets, q_terms, q_weights, k, strategy, q_filter, sort=sort, cursors=cursors,
                         collapse=collapse, **plans)
        try:
            b.run()
            return b.fetch() + (b.collapse_groups(),)
        finally:
            b.close()

    def search_plan(self, q_offsets, q_terms, q_weights, k: int, q_leaf=None, q_plan=None,
                    q_tie=None, q_nleaves=None, strategy: int = Wand, q_filter=None, **tree):
        """Batch search with score plans (multi-field leaves / DisMax; **tree: the two-level plan
        arrays of prepare()) -> (doc, seg, score, count)."""
        b = self.prepare(q_offsets, q_terms, q_weights, k, strategy, q_filter, q_leaf, q_plan,
                         q_tie, q_nleaves, **tree)
        try:
            b.run()
            return b.fetch()
        finally:
            b.close()

    def search_batch(self, q_offsets, q_terms, q_weights, k: int, strategy: int = Wand,
                     want_stats: bool = False, q_filter=None):
        """One-shot slg_search_batch over CSR queries -> (doc, seg, score, count[, stats]).
        q_filter: optional int array, one filter id per query (< 0: none)."""
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.uint32)
        nq = len(q_offsets) - 1
        q_terms = np.ascontiguousarray(q_terms, dtype=np.uint32).reshape(-1, self.n_segs)
        q_weights = np.ascontiguousarray(q_weights, dtype=np.float32)
        qs = (N.Query * max(nq, 1))()
        for q in range(nq):
            a, b = int(q_offsets[q]), int(q_offsets[q + 1])
            qs[q] = N.Query(b - a, q_terms.ctypes.data + a * self.n_segs * 4,
                            q_weights.ctypes.data + a * 4)
        out_doc = np.zeros((nq, k), dtype=np.uint32)
        out_seg = np.zeros((nq, k), dtype=np.uint32)
        out_score = np.zeros((nq, k), dtype=np.float32)
        out_count = np.zeros(nq, dtype=np.uint32)
        stats = (N.Stats * max(nq, 1))() if want_stats else None
        qf = None if q_filter is None else np.ascontiguousarray(q_filter, dtype=np.int32)
        assert qf is None or len(qf) == nq
        N.check(self._lib.slg_search_batch_filtered(
            self._h, qs, nq, None if qf is None else _ptr(qf), k, strategy, _ptr(out_doc),
            _ptr(out_seg), _ptr(out_score), _ptr(out_count),
            None if stats is None else C.addressof(stats)))
        if want_stats:
            return out_doc, out_seg, out_score, out_count, stats
        return out_doc, out_seg, out_score, out_count

    def execute_top_k(self, terms: Sequence[Tuple[int, float]], k: int, strategy: int = Wand,
                      segment: int = 0) -> List[Tuple[int, float]]:
        """query/wand.rs:338-356 for one query against one segment: terms = [(term_id, weight)],
        term i is leaf i.  Returns [(doc_id, score)] sorted score desc, doc asc."""
        ids = np.full((len(terms), self.n_segs), N.NO_TERM, dtype=np.uint32)
        for i, (tid, _) in enumerate(terms):
            ids[i, segment] = tid
        w = np.array([t[1] for t in terms], dtype=np.float32)
        offs = np.array([0, len(terms)], dtype=np.uint32)
        d, s, sc, c = self.search_batch(offs, ids, w, k, strategy)
        return [(int(d[0, i]), float(sc[0, i])) for i in range(int(c[0]))]

    def search(self, query: str, default_field: str, limit: int = 10, strategy: int = Wand):
        """IndexReader::search for an eligible query string: k = limit + 1 is handed to the
        scorer (api/reader.rs:2615-2619), hits truncated to limit (:2836-2852).
        Returns [(segment_ord, doc_id, score)]."""
        folded = fold_terms(parse_query_terms(query, default_field))
        if not folded:
            return []
        ids, w = resolve_query(self.segments, folded)
        offs = np.array([0, len(folded)], dtype=np.uint32)
        d, s, sc, c = self.search_batch(offs, ids, w, limit + 1, strategy)
        n = min(int(c[0]), limit)
        return [(int(s[0, i]), int(d[0, i]), float(sc[0, i])) for i in range(n)]

    def search_planned(self, planned, plan: int, n_leaves: int, tie_breaker: float = 0.0,
                       limit: int = 10, strategy: int = Wand, filter_id: int = -1):
        """One request whose scored terms come from segment.plan_query_string / plan_best_fields /
        plan_most_fields / plan_dis_max_terms (the leaf assignment of query/planner.rs).
        Returns [(segment_ord, doc_id, score)] like search()."""
        from .segment import resolve_plan
        if not planned:
            return []
        ids, w, leaf = resolve_plan(self.segments, planned)
        offs = np.array([0, len(planned)], dtype=np.uint32)
        d, s, sc, c = self.search_plan(offs, ids, w, limit + 1, q_leaf=leaf, q_plan=[plan],
                                       q_tie=[tie_breaker], q_nleaves=[n_leaves], strategy=strategy,
                                       q_filter=None if filter_id < 0 else [filter_id])
        n = min(int(c[0]), limit)
        return [(int(s[0, i]), int(d[0, i]), float(sc[0, i])) for i in range(n)]

    # -- rerank ----------------------------------------------------------------------
    def _rerank(self, entry, nq: int, lead, cand_doc, cand_seg, cand_bm25, cand_count, k_out: int):
        """One host-array rerank entry: entry(index, nq, *lead, candidates, max_cand, k_out, outputs).
        -> (out_doc, out_seg, out_score, out_vec, out_count)."""
        cand_doc = np.ascontiguousarray(cand_doc, dtype=np.uint32).reshape(nq, -1)
        max_cand = cand_doc.shape[1]
        cand_seg = np.ascontiguousarray(cand_seg, dtype=np.uint32).reshape(nq, max_cand)
        cand_bm25 = np.ascontiguousarray(cand_bm25, dtype=np.float32).reshape(nq, max_cand)
        cand_count = np.ascontiguousarray(cand_count, dtype=np.uint32)
        out = (np.zeros((nq, k_out), dtype=np.uint32), np.zeros((nq, k_out), dtype=np.uint32),
               np.zeros((nq, k_out), dtype=np.float32), np.zeros((nq, k_out), dtype=np.float32),
               np.zeros(nq, dtype=np.uint32))
        N.check(entry(self._h, nq, *lead, _ptr(cand_doc), _ptr(cand_seg), _ptr(cand_bm25), _ptr(cand_count),
                      max_cand, k_out, *map(_ptr, out)))
        return out

    def rerank_batch(self, qvecs, alpha, cand_doc, cand_seg, cand_bm25, cand_count, k_out: int):
        """gpu::rerank slot (gpu/rerank.rs:3): vector similarity + alpha blend + top-k_out."""
        qvecs = np.ascontiguousarray(qvecs, dtype=np.float32)
        nq = qvecs.shape[0]
        alpha = _f32(alpha, (nq,))
        return self._rerank(self._lib.slg_rerank_batch, nq, (_ptr(qvecs), _ptr(alpha)),
                            cand_doc, cand_seg, cand_bm25, cand_count, k_out)

    def rerank_multi_batch(self, qvecs, alpha, cand_doc, cand_seg, cand_bm25, cand_count, k_out: int,
                           boost=None):
        """Hybrid rerank with several vector clauses (compute_hybrid_score, api/reader.rs:225-254):
        qvecs [nq, n_clauses, dim], alpha / boost [nq, n_clauses]."""
        qvecs = np.ascontiguousarray(qvecs, dtype=np.float32)
        nq, nc = qvecs.shape[0], qvecs.shape[1]
        alpha, bst = _f32(alpha, (nq, nc)), _f32(boost, (nq, nc))
        return self._rerank(self._lib.slg_rerank_multi_batch, nq, (nc, _ptr(qvecs), _ptr(alpha), _ptr(bst)),
                            cand_doc, cand_seg, cand_bm25, cand_count, k_out)

    def add_vector_field(self, per_segment) -> int:
        """Stage one more vector field (vectors/mod.rs:10-17: a VectorStore per field).  per_segment[s]
        = (metric, vec_offsets u32[n_docs], vec_values f32[rows, dim]) or None (segment s has no
        vectors in it).  -> field id (>= 1; 0 is the field of the segment descriptors)."""
        descs = (N.VectorFieldDesc * len(per_segment))()
        keep = []
        for s, f in enumerate(per_segment):
            if f is None:
                continue
            metric, offs, vals = f
            offs = np.ascontiguousarray(offs, dtype=np.uint32)
            vals = np.ascontiguousarray(vals, dtype=np.float32)
            keep += [offs, vals]
            descs[s].vec_dim, descs[s].vec_metric = vals.shape[1], int(metric)
            descs[s].vec_offsets, descs[s].vec_values = offs.ctypes.data, vals.ctypes.data
            descs[s].vec_rows = vals.shape[0]
        rc = self._lib.slg_index_add_vector_field(self._h, C.addressof(descs), len(per_segment))
        if rc < 0:
            N.check(rc)
        return rc

    def rerank_fields_batch(self, clause_field, qvecs, alpha, cand_doc, cand_seg, cand_bm25, cand_count,
                            k_out: int, boost=None):
        """Hybrid rerank whose clauses name different vector fields (api/reader.rs:225-254).
        clause_field [n_clauses] field ids; qvecs [nq, sum of the clause dims] (a query's clause
        vectors one after another); alpha / boost [nq, n_clauses]."""
        cf = np.ascontiguousarray(clause_field, dtype=np.uint32)
        nc = len(cf)
        qvecs = np.ascontiguousarray(qvecs, dtype=np.float32)
        nq = qvecs.shape[0]
        alpha, bst = _f32(alpha, (nq, nc)), _f32(boost, (nq, nc))
        return self._rerank(self._lib.slg_rerank_fields_batch, nq,
                            (nc, _ptr(cf), _ptr(qvecs), _ptr(alpha), _ptr(bst)),
                            cand_doc, cand_seg, cand_bm25, cand_count, k_out)

    def vector_search(self, clause_field, qvecs, alpha, cand_size: int, k_out: int, boost=None, q_filter=None):
        """Exact vector-only search (search_vector_only, api/reader.rs:2187-2330) over every stored
        vector.  clause_field [n_clauses] field ids; qvecs [nq, sum of the clause dims] (a query's
        clause vectors one after another); alpha / boost [nq, n_clauses]; q_filter [nq] filter ids
        (< 0: none).  -> (doc, seg, score, vec_score) [nq, k_out], count [nq], total [nq] (union size)."""
        return self._vector_call(self._lib.slg_vector_search_batch, clause_field, qvecs, alpha, boost, q_filter,
                                 (cand_size,), k_out)

    def _vector_call(self, fn, clause_field, qvecs, alpha, boost, q_filter, ints, k_out, text=None):
        """One host-array call of the vector search family: stage the clause arrays and the filter ids, allocate
        the six outputs and call fn with `ints` (cand_size and the call's own integer) before k_out.  text: the
        hybrid call's (q_offsets, q_terms, q_weights, k, strategy), which fn takes ahead of the clause arrays."""
        cf = np.ascontiguousarray(clause_field, dtype=np.uint32)
        nc = len(cf)
        qvecs = np.ascontiguousarray(qvecs, dtype=np.float32)
        nq = qvecs.shape[0] if text is None else len(text[0]) - 1
        alpha, bst = _f32(alpha, (nq, nc)), _f32(boost, (nq, nc))
        flt = None if q_filter is None else np.ascontiguousarray(q_filter, dtype=np.int32)
        clause = (nc, _ptr(cf), _ptr(qvecs), _ptr(alpha), _ptr(bst))
        if text is None:
            head = clause + (_ptr(flt),)
        else:
            head = tuple(_ptr(x) for x in text[:3]) + (None, _ptr(flt), int(text[3]), int(text[4])) + clause
        doc = np.zeros((nq, k_out), np.uint32)
        seg = np.zeros((nq, k_out), np.uint32)
        score = np.zeros((nq, k_out), np.float32)
        vec = np.zeros((nq, k_out), np.float32)
        count = np.zeros(nq, np.uint32)
        total = np.zeros(nq, np.uint64)
        N.check(fn(self._h, nq, *head, *(int(i) for i in ints), int(k_out),
                   _ptr(doc), _ptr(seg), _ptr(score), _ptr(vec), _ptr(count), _ptr(total)))
        return doc, seg, score, vec, count, total

    def _vector_call_device(self, fn, nq, clause_field, d_in, ints, k_out, d_out) -> None:
        """One device-pointer call of the family: d_in = (d_qvecs, d_alpha, d_boost, d_q_filter), d_out the six
        output pointers; clause_field stays a host array."""
        cf = np.ascontiguousarray(clause_field, dtype=np.uint32)
        N.check(fn(self._h, nq, len(cf), _ptr(cf), *d_in, *(int(i) for i in ints), int(k_out), *d_out))

    def quantize_vector_field(self, field: int = 0) -> None:
        """Build the bf16 copy of vector field `field` on the device (slg_index_quantize_vector_field): what
        vector_search_approx scans.  A second call for the same field does nothing."""
        N.check(self._lib.slg_index_quantize_vector_field(self._h, int(field)))

    def fetch_vector_copy(self, field: int, seg: int, dim: int):
        """The bf16 copy of segment `seg`'s store of `field` (slg_index_fetch_vector_copy): (bf16 bit patterns
        u16 [rows, dim], f32 squared norms [rows]), or None when the segment has no vectors in the field.  dim:
        the field's dimension in that segment."""
        rows = self._lib.slg_index_fetch_vector_copy(self._h, int(field), int(seg), None, None, 0)
        if rows < 0:
            N.check(rows)
        if rows == 0:
            return None
        bits = np.zeros((rows, int(dim)), np.uint16)
        norms = np.zeros(rows, np.float32)
        rc = self._lib.slg_index_fetch_vector_copy(self._h, int(field), int(seg), _ptr(bits), _ptr(norms), rows)
        if rc < 0:
            N.check(rc)
        return bits, norms

    def vector_search_approx(self, clause_field, qvecs, alpha, cand_size: int, refine: int, k_out: int, boost=None,
                             q_filter=None):
        """Two-pass vector search (slg_vector_search_batch_approx): per clause the best `refine` docs of a scan of
        the field's bf16 copy (quantize_vector_field) are scored again from the f32 store, and the best cand_size
        of those form the clause's list.  Arguments and result as vector_search(); every returned score is the
        exact call's, and refine >= the live docs with a vector makes the whole result the exact call's."""
        return self._vector_call(self._lib.slg_vector_search_batch_approx, clause_field, qvecs, alpha, boost, q_filter,
                                 (cand_size, refine), k_out)

    def vector_search_approx_device(self, nq, clause_field, d_qvecs, d_alpha, d_boost, d_q_filter, cand_size, refine,
                                    k_out, d_out_doc, d_out_seg, d_out_score, d_out_vec, d_out_count,
                                    d_out_total) -> None:
        """Device-pointer form of vector_search_approx (ints; d_boost / d_q_filter may be None; clause_field
        stays a host array), asynchronous on the index stream."""
        self._vector_call_device(self._lib.slg_vector_search_batch_approx_device, nq, clause_field,
                                 (d_qvecs, d_alpha, d_boost, d_q_filter), (cand_size, refine), k_out,
                                 (d_out_doc, d_out_seg, d_out_score, d_out_vec, d_out_count, d_out_total))

    def cluster_vector_field(self, field: int, per_segment) -> None:
        """Build the inverted-file lists of vector field `field` on the device (slg_index_cluster_vector_field):
        what vector_search_ivf probes.  per_segment[s] = the segment's centroids f32 [n_lists, dim], None (the
        segment is or becomes unclustered) or N.KEEP_VECTOR_LISTS (its lists stay as they are)."""
        descs = (N.VectorListsDesc * max(len(per_segment), 1))()
        keep = []
        for s, c in enumerate(per_segment):
            if c is None:
                descs[s].n_lists, descs[s].centroids = 0, None
            elif isinstance(c, int):
                descs[s].n_lists, descs[s].centroids = int(c), None
            else:
                c = np.ascontiguousarray(c, dtype=np.float32)
                keep.append(c)
                descs[s].n_lists, descs[s].centroids = c.shape[0], c.ctypes.data
        N.check(self._lib.slg_index_cluster_vector_field(self._h, int(field), C.addressof(descs), len(per_segment)))

    def train_vector_field(self, field: int, per_segment, dim=None):
        """Train the centroids of vector field `field` on the device and build its lists around them
        (slg_index_train_vector_field): Lloyd steps over each segment's own f32 store.  per_segment[s] = None (the
        segment is or becomes unclustered), N.KEEP_VECTOR_LISTS (its lists stay as they are), (n_lists, iters) (the
        start is rows of the store) or (n_lists, iters, init f32 [n_lists, dim]).  The library reads n_lists * dim
        floats of an init, so its width must be the field's dimension: it is checked against `dim` when that is
        given, and for field 0 against the segment's own vec_dim.
        -> per segment dict(iters_run, moved, empty_lists, max_len); zeros for a segment that was not trained."""
        import numbers
        n = len(per_segment)
        descs = (N.VectorTrainDesc * max(n, 1))()
        stats = (N.VectorTrainStats * max(n, 1))()
        keep = []
        for s, c in enumerate(per_segment):
            if c is None:
                descs[s].n_lists, descs[s].iters, descs[s].init = 0, 0, None
            elif isinstance(c, numbers.Integral):
                descs[s].n_lists, descs[s].iters, descs[s].init = int(c), 0, None
            else:
                descs[s].n_lists, descs[s].iters, descs[s].init = int(c[0]), int(c[1]), None
                if len(c) > 2 and c[2] is not None:
                    init = np.ascontiguousarray(c[2], dtype=np.float32)
                    if init.ndim != 2 or init.shape[0] != int(c[0]):
                        raise ValueError("init must be f32 [n_lists, dim]")
                    want = dim
                    if want is None and int(field) == 0 and s < len(self.segments):
                        want = getattr(self.segments[s], "vec_dim", 0) or None
                    if want is not None and init.shape[1] != int(want):
                        raise ValueError(f"init of segment {s} has {init.shape[1]} columns, the field's dimension "
                                         f"is {int(want)}")
                    keep.append(init)
                    descs[s].init = init.ctypes.data
        N.check(self._lib.slg_index_train_vector_field(self._h, int(field), C.addressof(descs), n,
                                                       C.addressof(stats)))
        return [dict(iters_run=int(st.iters_run), moved=int(st.moved), empty_lists=int(st.empty_lists),
                     max_len=int(st.max_len)) for st in stats[:n]]

    def fetch_vector_lists(self, field: int, seg: int, dim: int):
        """The lists of segment `seg` in `field` (slg_index_fetch_vector_lists): (list_begin u32 [n_lists + 1],
        docs u32 [list_begin[-1]], centroids f32 [n_lists, dim]), or None when the segment is unclustered or has
        no vectors in the field.  dim: the field's dimension."""
        n = self._lib.slg_index_fetch_vector_lists(self._h, int(field), int(seg), None, None, None, 0, 0)
        if n < 0:
            N.check(n)
        if n == 0:
            return None
        begin = np.zeros(n + 1, np.uint32)
        cents = np.zeros((n, int(dim)), np.float32)
        rc = self._lib.slg_index_fetch_vector_lists(self._h, int(field), int(seg), _ptr(begin), None, _ptr(cents), n, 0)
        if rc < 0:
            N.check(rc)
        docs = np.zeros(int(begin[-1]), np.uint32)
        if len(docs):
            rc = self._lib.slg_index_fetch_vector_lists(self._h, int(field), int(seg), _ptr(begin), _ptr(docs),
                                                        _ptr(cents), n, len(docs))
            if rc < 0:
                N.check(rc)
        return begin, docs, cents

    def vector_search_ivf(self, clause_field, qvecs, alpha, cand_size: int, nprobe: int, k_out: int, boost=None,
                          q_filter=None):
        """Vector search over the fields' inverted-file lists (slg_vector_search_batch_ivf): per clause the docs
        of the `nprobe` lists nearest the query (cluster_vector_field) and of the unclustered segments are scored
        from the f32 store, and the best cand_size form the clause's list.  Arguments and result as
        vector_search(); every returned score is the exact call's, and nprobe >= the lists of every clause's
        field makes the whole result the exact call's.  cand_size <= 64."""
        return self._vector_call(self._lib.slg_vector_search_batch_ivf, clause_field, qvecs, alpha, boost, q_filter,
                                 (cand_size, nprobe), k_out)

    def vector_search_ivf_device(self, nq, clause_field, d_qvecs, d_alpha, d_boost, d_q_filter, cand_size, nprobe,
                                 k_out, d_out_doc, d_out_seg, d_out_score, d_out_vec, d_out_count,
                                 d_out_total) -> None:
        """Device-pointer form of vector_search_ivf (ints; d_boost / d_q_filter may be None; clause_field stays a
        host array), asynchronous on the index stream."""
        self._vector_call_device(self._lib.slg_vector_search_batch_ivf_device, nq, clause_field,
                                 (d_qvecs, d_alpha, d_boost, d_q_filter), (cand_size, nprobe), k_out,
                                 (d_out_doc, d_out_seg, d_out_score, d_out_vec, d_out_count, d_out_total))

    def search_hybrid(self, q_offsets, q_terms, q_weights, k: int, clause_field, qvecs, alpha, cand_size: int,
                      k_out: int, boost=None, strategy: int = Wand, q_filter=None, **plans):
        """Hybrid text + vector search (merge_vector_hits, api/reader.rs:2474-2537) in one call: the BM25 top k
        of the text query's matched docs, per clause the best cand_size vector scores among the matched docs,
        their union blended as compute_hybrid_score.  Queries as prepare(); clause arrays as vector_search().
        -> (doc, seg, score, vec_score) [nq, k_out], count [nq], total [nq] (union size)."""
        if plans:  # (score plans: the prepared form builds slg_score_plans)
            with self.prepare(q_offsets, q_terms, q_weights, k, strategy, q_filter, hybrid=True, **plans) as b:
                return b.hybrid(clause_field, qvecs, alpha, cand_size, k_out, boost)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.uint32)
        q_terms = np.ascontiguousarray(q_terms, dtype=np.uint32)
        q_weights = np.ascontiguousarray(q_weights, dtype=np.float32)
        return self._vector_call(self._lib.slg_search_batch_hybrid, clause_field, qvecs, alpha, boost, q_filter,
                                 (cand_size,), k_out, text=(q_offsets, q_terms, q_weights, k, strategy))

    def vector_search_device(self, nq, clause_field, d_qvecs, d_alpha, d_boost, d_q_filter, cand_size, k_out,
                             d_out_doc, d_out_seg, d_out_score, d_out_vec, d_out_count, d_out_total) -> None:
        """Device-pointer form of vector_search (ints; d_boost / d_q_filter may be None; clause_field
        stays a host array), asynchronous on the index stream."""
        self._vector_call_device(self._lib.slg_vector_search_batch_device, nq, clause_field,
                                 (d_qvecs, d_alpha, d_boost, d_q_filter), (cand_size,), k_out,
                                 (d_out_doc, d_out_seg, d_out_score, d_out_vec, d_out_count, d_out_total))

    def rerank_batch_device(self, nq, d_qvecs, d_alpha, d_cand_doc, d_cand_seg, d_cand_bm25,
                            d_cand_count, max_cand, k_out, d_out_doc, d_out_seg, d_out_score,
                            d_out_vec, d_out_count) -> None:
        """Device-pointer form (ints), asynchronous on the index stream."""
        N.check(self._lib.slg_rerank_batch_device(
            self._h, nq, d_qvecs, d_alpha, d_cand_doc, d_cand_seg, d_cand_bm25, d_cand_count,
            max_cand, k_out, d_out_doc, d_out_seg, d_out_score, d_out_vec, d_out_count))

    def rerank_multi_batch_device(self, nq, n_clauses, d_qvecs, d_alpha, d_boost, d_cand_doc, d_cand_seg,
                                  d_cand_bm25, d_cand_count, max_cand, k_out, d_out_doc, d_out_seg,
                                  d_out_score, d_out_vec, d_out_count) -> None:
        """Device-pointer form of rerank_multi_batch (d_qvecs [nq, n_clauses, dim]; d_boost may be
        None), asynchronous on the index stream.  >= 2 cosine clauses run on the matrix cores."""
        N.check(self._lib.slg_rerank_multi_batch_device(
            self._h, nq, n_clauses, d_qvecs, d_alpha, d_boost, d_cand_doc, d_cand_seg, d_cand_bm25,
            d_cand_count, max_cand, k_out, d_out_doc, d_out_seg, d_out_score, d_out_vec, d_out_count))

    def merge_shards_device(self, n_shards, nq, k, d_doc, d_seg, d_score, d_count, seg_stride,
                            d_out_doc, d_out_seg, d_out_score, d_out_count) -> None:
        N.check(self._lib.slg_merge_shards_device(self._h, n_shards, nq, k, d_doc, d_seg, d_score,
                                                  d_count, seg_stride, d_out_doc, d_out_seg,
                                                  d_out_score, d_out_count))


def expand_request(kind: int, field: str, term: str, max_expansions: int, max_edits: int = 0, prefix_length: int = 0,
                   min_length: int = 0) -> dict:
    """One request of GpuIndex.expand(): kind N.EXPAND_FUZZY (term: the analysed term; the FuzzyOptions),
    N.EXPAND_PREFIX (term: the prefix), N.EXPAND_WILDCARD or N.EXPAND_REGEX (term: the pattern)."""
    return dict(kind=kind, field=field, term=term, max_expansions=max_expansions, max_edits=max_edits,
                prefix_length=prefix_length, min_length=min_length)


FUZZY_DEFAULTS = dict(max_edits=1, prefix_length=1, max_expansions=50, min_length=3)  # FuzzyOptions::default


def suggest_request(field: str, term: str, size: int = 5, fuzzy: Optional[dict] = None) -> dict:
    """One request of GpuIndex.suggest() (SuggestRequest::Completion): term is the analysed completion input
    (completion_input()); fuzzy None, or a dict of FuzzyOptions over the defaults 1 / 1 / 50 / 3 (max_edits,
    prefix_length, max_expansions, min_length)."""
    return dict(field=field, term=term, size=size, fuzzy=None if fuzzy is None else dict(FUZZY_DEFAULTS, **fuzzy))


def completion_input(kind: str, prefix: str) -> str:
    """completion_inputs (api/reader.rs:1915-1939) for what the user typed: kind "keyword" lowercases ASCII letters
    (to_ascii_lowercase); kind "text" expects `prefix` already analysed by the caller's search analyzer and takes
    its last whitespace token, or the prefix itself if there is none."""
    if kind == "keyword":
        return "".join(chr(ord(c) + 32) if "A" <= c <= "Z" else c for c in prefix)
    if kind == "text":
        tokens = prefix.split()
        return tokens[-1] if tokens else prefix
    raise ValueError("completion suggest is only supported on text / keyword fields")


def fold_expansions(nq: int, source_query, source_key, rows, n_segs: int, boost=1.0, names=None):
    """Expansions into the arrays of a plain batch with plans.  Source term i belongs to query source_query[i]
    (ascending), has the exact key source_key[i] and expanded to rows[i] = (term_id_rows, distances); it is one leaf
    of its query.  A key's weight is boost * 1 / (distance + 1) in f32 (boost: one for all, or one per source term);
    equal keys of a query fold by summing and
    keep their first leaf (api/reader.rs:2971-2983); leaves a fold left without a term are dropped.
    -> (q_offsets, q_terms, q_weights, plans dict for search_plan)."""
    offs = [0]
    terms, weights, leaves, nleaves = [], [], [], []
    boosts = np.broadcast_to(np.asarray(boost, dtype=np.float32), (len(source_query),))
    i = 0
    for q in range(nq):
        slot = {}   # key identity -> index into this query's lists
        q_rows, q_w, q_leaf = [], [], []
        leaf = 0
        while i < len(source_query) and source_query[i] == q:
            ids, dist = rows[i]
            for r in range(len(dist)):
                present = bool((ids[r] != N.NO_TERM).any())
                # a key no segment holds can only be the source's own exact key (row 0)
                ident = ids[r].tobytes() if present else ("absent", source_key[i])
                w = boosts[i] * (np.float32(1.0) / (np.float32(int(dist[r])) + np.float32(1.0)))
                if ident in slot:
                    q_w[slot[ident]] = np.float32(q_w[slot[ident]] + w)
                else:
                    slot[ident] = len(q_rows)
                    q_rows.append(ids[r])
                    q_w.append(np.float32(w))
                    q_leaf.append(leaf)
            leaf += 1
            i += 1
        if len(q_rows) > N.MAX_QUERY_TERMS:
            name = f" ({names[q]!r})" if names is not None else ""
            raise N.SlgError(N.ERR_UNSUPPORTED, f"query {q}{name} folds to {len(q_rows)} terms, more than "
                                                f"SLG_MAX_QUERY_TERMS = {N.MAX_QUERY_TERMS}: CPU path")
        dense = {l: j for j, l in enumerate(sorted(set(q_leaf)))}
        terms += q_rows
        weights += q_w
        leaves += [dense[l] for l in q_leaf]
        nleaves.append(len(dense))
        offs.append(len(terms))
    q_terms = np.array(terms, dtype=np.uint32).reshape(-1, n_segs)
    plans = dict(q_leaf=np.array(leaves, dtype=np.uint32), q_plan=np.full(nq, N.PLAN_SUM, dtype=np.uint32),
                 q_tie=np.zeros(nq, dtype=np.float32), q_nleaves=np.array(nleaves, dtype=np.uint32))
    return np.array(offs, dtype=np.uint32), q_terms, np.array(weights, dtype=np.float32), plans


def shard_unique_id() -> bytes:
    """slg_shard_unique_id: the 128-byte id rank 0 creates and hands to the other ranks of a shard
    group out of band (ncclGetUniqueId)."""
    buf = C.create_string_buffer(N.SHARD_UNIQUE_ID_BYTES)
    N.check(N.load().slg_shard_unique_id(buf, N.SHARD_UNIQUE_ID_BYTES))
    return buf.raw


class ShardGroup:
    """This rank's membership in an index-sharded search (slg_shard_group): its GpuIndex holds the
    segments of shard `rank`; the RCCL communicator lives behind the C ABI, no torch involved.
    Creation is collective: every rank constructs its ShardGroup with the same unique_id."""

    def __init__(self, index: GpuIndex, rank: int, world: int, unique_id: bytes, segs_per_rank: Optional[int] = None):
        self.index, self.rank, self.world = index, rank, world
        self.segs_per_rank = index.n_segs if segs_per_rank is None else int(segs_per_rank)
        self._lib = index._lib
        assert len(unique_id) == N.SHARD_UNIQUE_ID_BYTES
        self._h = self._lib.slg_shard_group_create(index._h, rank, world, unique_id, self.segs_per_rank)
        if not self._h:
            raise N.SlgError(N.last_error_code() or N.ERR_INVALID, N.last_error())

    def stats(self) -> dict:
        """slg_shard_group_stats (with GpuIndex.profile(True)): mean device ms per sharded run fetched
        since the last call — this rank's kernels, the all-gather, the merge."""
        a, b, c, n = C.c_double(), C.c_double(), C.c_double(), C.c_uint64()
        N.check(self._lib.slg_shard_group_stats(self._h, C.addressof(a), C.addressof(b), C.addressof(c), C.addressof(n)))
        d = max(1, n.value)
        return {"runs": int(n.value), "kernel_ms": a.value / d, "gather_ms": b.value / d, "merge_ms": c.value / d}

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.slg_shard_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def sort_spec(sort) -> "N.SortSpec":
    """[(field, order)] -> slg_sort_spec: field = sort field id or "_score" (N.SORT_SCORE), order = "asc" /
    "desc" (or N.ORDER_*).  More than N.MAX_SORT_PARTS parts are passed on as given (the library refuses
    them)."""
    spec = N.SortSpec()
    spec.n_parts = len(sort)
    for i, (field, order) in enumerate(sort[:N.MAX_SORT_PARTS]):
        spec.field[i] = N.SORT_SCORE if field == "_score" else int(field)
        spec.order[i] = {"asc": N.ORDER_ASC, "desc": N.ORDER_DESC}.get(order, order)
    return spec


def collapse_spec(collapse: dict):
    """The dict of GpuIndex.search_collapse as (N.CollapseSpec, the inner sort spec it points to or None)."""
    inner = collapse.get("inner_sort")
    keep = None if inner is None else (inner if isinstance(inner, N.SortSpec) else sort_spec(inner))
    spec = N.CollapseSpec(int(collapse["field"]), int(collapse["group_limit"]), int(collapse.get("inner_from", 0)),
                          int(collapse.get("inner_size", 0)), None if keep is None else C.addressof(keep))
    return spec, keep


def rescore_spec(rescore: dict, nq: int):
    """The dict of GpuIndex.search_rescore as (N.RescoreSpec, the arrays it points into)."""
    def arr(name, dtype, per_query=False):
        a = rescore.get(name)
        if a is None:
            return None
        a = np.asarray(a, dtype=dtype)
        if per_query and a.ndim == 0:
            a = np.full(nq, a, dtype=dtype)
        return np.ascontiguousarray(a)
    keep = [arr("q_offsets", np.uint32), arr("q_terms", np.uint32), arr("q_weights", np.float32),
            arr("q_leaf", np.uint32), arr("q_plan", np.int32, True), arr("q_tie", np.float32, True),
            arr("q_nleaves", np.uint32, True), arr("q_min_match", np.uint32, True),
            arr("window", np.uint32, True), arr("mode", np.int32, True)]
    assert keep[0] is not None and len(keep[0]) == nq + 1 and keep[8] is not None
    assert all(a is None or len(a) == nq for a in keep[4:])
    return N.RescoreSpec(*[_ptr(a) for a in keep]), keep


def bool_spec(clauses: dict, nq: int):
    """The dict of GpuIndex.search_batch_bool as (N.BoolSpec, the arrays it points into)."""
    def arr(name, dtype, per_query=False):
        a = clauses.get(name)
        if a is None:
            return None
        a = np.asarray(a, dtype=dtype)
        if per_query and a.ndim == 0:
            a = np.full(nq, a, dtype=dtype)
        return np.ascontiguousarray(a)
    keep = [arr("c_offsets", np.uint32), arr("c_terms", np.uint32), arr("c_group", np.uint32),
            arr("g_offsets", np.uint32), arr("g_kind", np.int32), arr("q_min_should", np.uint32, True)]
    assert keep[0] is not None and len(keep[0]) == nq + 1 and keep[3] is not None and len(keep[3]) == nq + 1
    assert keep[5] is None or len(keep[5]) == nq
    return N.BoolSpec(*[_ptr(a) for a in keep]), keep


def bool_tree_spec(tree: dict, nq: int):
    """The dict of GpuIndex.search_batch_bool_tree (booltree.compile_matchers) as (N.BoolTreeSpec, the arrays it
    points into)."""
    def arr(name, dtype):
        a = tree.get(name)
        return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=dtype))
    keep = [arr("c_offsets", np.uint32), arr("c_terms", np.uint32), arr("c_group", np.uint32),
            arr("g_offsets", np.uint32), arr("f_offsets", np.uint32), arr("f_filter", np.int32),
            arr("n_offsets", np.uint32), arr("n_min_should", np.uint32), arr("e_offsets", np.uint32),
            arr("e_child", np.uint32), arr("e_kind", np.int32)]
    assert all(a is None or len(a) == nq + 1 for a in (keep[0], keep[3], keep[4], keep[6]))
    return N.BoolTreeSpec(*[_ptr(a) for a in keep]), keep


def phrase_spec(phrases: dict, nq: int):
    """The dict of GpuIndex.search_batch_phrase as (N.PhraseSpec, the arrays it points into)."""
    def arr(name, dtype, per_query=False):
        a = phrases.get(name)
        if a is None:
            return None
        a = np.asarray(a, dtype=dtype)
        if per_query and a.ndim == 0:
            a = np.full(nq, a, dtype=dtype)
        return np.ascontiguousarray(a)
    keep = [arr("p_offsets", np.uint32), arr("p_kind", np.int32), arr("p_slop", np.uint32), arr("v_offsets", np.uint32),
            arr("t_offsets", np.uint32), arr("t_terms", np.uint32), arr("q_min_should", np.uint32, True)]
    assert keep[0] is not None and len(keep[0]) == nq + 1
    assert keep[6] is None or len(keep[6]) == nq
    return N.PhraseSpec(*[_ptr(a) for a in keep]), keep


FSCORE_KINDS = {"weight": N.FSCORE_WEIGHT, "field_value_factor": N.FSCORE_FIELD_VALUE_FACTOR, "decay": N.FSCORE_DECAY}
FSCORE_MODIFIERS = {"none": N.FSCORE_MOD_NONE, "log": N.FSCORE_MOD_LOG, "log1p": N.FSCORE_MOD_LOG1P,
                    "log2p": N.FSCORE_MOD_LOG2P, "sqrt": N.FSCORE_MOD_SQRT, "reciprocal": N.FSCORE_MOD_RECIPROCAL}
FSCORE_DECAYS = {"exp": N.FSCORE_DECAY_EXP, "gauss": N.FSCORE_DECAY_GAUSS, "linear": N.FSCORE_DECAY_LINEAR}
FSCORE_MODES = {"sum": N.FSCORE_MODE_SUM, "multiply": N.FSCORE_MODE_MULTIPLY, "max": N.FSCORE_MODE_MAX,
                "min": N.FSCORE_MODE_MIN, "avg": N.FSCORE_MODE_AVG}
FSCORE_BOOSTS = {"multiply": N.FSCORE_BOOST_MULTIPLY, "sum": N.FSCORE_BOOST_SUM, "replace": N.FSCORE_BOOST_REPLACE,
                 "max": N.FSCORE_BOOST_MAX, "min": N.FSCORE_BOOST_MIN}


def fscore_spec(functions, nq: int):
    """One function_score per query as (N.FscoreSpec, the arrays it points into).  functions[q]: None (the query
    is left as it is) or a dict with `functions` (a list, in request order), `score_mode` ("multiply"), `boost_mode`
    ("multiply"), `max_boost` (None), `min_score` (None) and `boost` (1.0) — the request's defaults.  A function
    is a dict with `kind` ("weight" / "field_value_factor" / "decay") and `filter` (a filter id, default -1), plus
    weight: `weight`; field_value_factor: `field` (agg field id), `factor` (1.0), `modifier` ("none"), `missing`
    (0.0); decay: `field`, `origin`, `scale`, `offset` (0.0), `decay` (0.5), `function` ("exp").  Names may also be
    the numbers of N.FSCORE_*."""
    assert len(functions) == nq
    num = lambda table, v: table.get(v, v) if isinstance(v, str) else int(v)
    q = dict(off=[0], sm=[], bm=[], flags=[], maxb=[], mins=[], boost=[])
    f = dict(kind=[], field=[], filt=[], w=[], mod=[], dfn=[], missing=[], origin=[], scale=[], offset=[], decay=[])
    for fsq in functions:
        fsq = fsq or {}
        for fn in fsq.get("functions", ()):
            kind = num(FSCORE_KINDS, fn["kind"])
            f["kind"].append(kind)
            f["field"].append(int(fn.get("field", -1)))
            f["filt"].append(int(fn.get("filter", -1)))
            f["w"].append(fn["weight"] if kind == N.FSCORE_WEIGHT else fn.get("factor", 1.0))
            f["mod"].append(num(FSCORE_MODIFIERS, fn.get("modifier", "none")))
            f["dfn"].append(num(FSCORE_DECAYS, fn.get("function", "exp")))
            f["missing"].append(fn.get("missing", 0.0))
            f["origin"].append(fn.get("origin", 0.0))
            f["scale"].append(fn.get("scale", 1.0))
            f["offset"].append(fn.get("offset", 0.0))
            f["decay"].append(fn.get("decay", 0.5))
        q["off"].append(len(f["kind"]))
        q["sm"].append(num(FSCORE_MODES, fsq.get("score_mode", "multiply")))
        q["bm"].append(num(FSCORE_BOOSTS, fsq.get("boost_mode", "multiply")))
        maxb, mins = fsq.get("max_boost"), fsq.get("min_score")
        q["flags"].append((N.FSCORE_HAS_MAX_BOOST if maxb is not None else 0) | (N.FSCORE_HAS_MIN_SCORE if mins is not None else 0))
        q["maxb"].append(0.0 if maxb is None else maxb)
        q["mins"].append(0.0 if mins is None else mins)
        q["boost"].append(fsq.get("boost", 1.0))
    pad = lambda a, dt: np.ascontiguousarray(a if len(a) else [0], dtype=dt)  # (never NULL: an empty array is read nowhere)
    keep = [pad(q["off"], np.uint32), pad(q["sm"], np.int32), pad(q["bm"], np.int32), pad(q["flags"], np.uint32),
            pad(q["maxb"], np.float32), pad(q["mins"], np.float32), pad(q["boost"], np.float32),
            pad(f["kind"], np.int32), pad(f["field"], np.int32), pad(f["filt"], np.int32), pad(f["w"], np.float32),
            pad(f["mod"], np.int32), pad(f["dfn"], np.int32), pad(f["missing"], np.float64), pad(f["origin"], np.float64),
            pad(f["scale"], np.float64), pad(f["offset"], np.float64), pad(f["decay"], np.float64)]
    return N.FscoreSpec(*[_ptr(a) for a in keep]), keep


def sort_cursor(cursor, sort=None) -> "N.SortCursor":
    """None (a first page), an N.SortCursor, or (values, segment_ord, doc_id) -> slg_sort_cursor.  values: one
    per sort part (score order: one, the score): an int is an i64 value, a float an f64 value (or, on a
    `_score` part and in score order, an f32 score), None Missing."""
    c = N.SortCursor()
    if cursor is None:
        return c
    if isinstance(cursor, N.SortCursor):
        return cursor
    values, seg, doc = cursor
    c.has_cursor, c.segment_ord, c.doc_id = 1, int(seg), int(doc)
    parts = ["_score"] if sort is None else [p for p, _ in sort]
    for i, v in enumerate(values):
        if v is None:
            c.missing_mask |= 1 << i
        elif i < len(parts) and (parts[i] == "_score" or parts[i] == N.SORT_SCORE):
            c.value_bits[i] = struct.unpack("<I", struct.pack("<f", float(v)))[0]
        elif isinstance(v, float):
            c.value_bits[i] = struct.unpack("<Q", struct.pack("<d", v))[0]
        else:
            c.value_bits[i] = int(v) & 0xFFFFFFFFFFFFFFFF
    return c


def _addr(x):
    return None if x is None else C.addressof(x)


def _script_spec(script, nq: int):
    from .script import script_spec
    return script_spec(script, nq)


# argument of PreparedBatch -> (what makes (spec, the objects it points into) of it, the attribute that keeps those).
# The argument may be that pair already.
_SPEC_MAKERS = {
    "script": (_script_spec, "_script_keep"), "fscore": (fscore_spec, "_fscore_keep"),
    "collapse": (lambda collapse, nq: collapse_spec(collapse), "_collapse_keep"),
    "clause_tree": (bool_tree_spec, "_tree_keep"), "phrases": (phrase_spec, "_phrase_keep"),
    "clauses": (bool_spec, "_bool_keep"), "rescore": (rescore_spec, "_rescore_keep"),
}


class _BatchKind(NamedTuple):
    arg: Optional[str]  # the argument (or the spec an aggs.AggPlan carries) that asks for the kind; None: a plain batch
    entry: str          # its prepare call
    own: tuple          # what its pointers between q_filter and k are made from, in the call's order
    refuses: tuple = ()  # the arguments it is not built on ...
    message: str = ""    # ... and the ERR_UNSUPPORTED message that says so


_FAMILY_REFUSES = ("hybrid", "cursors", "rescore", "clauses", "phrases", "fscore", "collapse", "clause_tree", "script")
# in the precedence PreparedBatch gives them: the first kind that is asked for is the one prepared
_BATCH_KINDS = (
    _BatchKind("term_buckets", "slg_batch_prepare_term_buckets", ("sort", "agg_spec", "term_bucket_spec"),
               ("top_hits", "composite") + _FAMILY_REFUSES,
               "significant_terms and rare_terms are built on plain, sorted and aggregation batches only"),
    _BatchKind("composite", "slg_batch_prepare_composite", ("sort", "agg_spec", "composite_spec"),
               ("top_hits",) + _FAMILY_REFUSES, "composite is built on plain, sorted and aggregation batches only"),
    _BatchKind("top_hits", "slg_batch_prepare_top_hits", ("sort", "agg_spec", "top_hits_spec"), _FAMILY_REFUSES,
               "top_hits is built on plain, sorted and aggregation batches only"),
    _BatchKind("script", "slg_batch_prepare_script", ("sort", "script", "fscore", "script_order"),
               ("hybrid", "cursors", "aggs", "rescore", "clauses", "phrases", "collapse", "clause_tree"),
               "script_score is not built on cursor, hybrid, aggregation, rescore, bool, phrase, collapse or matcher "
               "tree batches"),
    _BatchKind("clause_tree", "slg_batch_prepare_bool_tree", ("sort", "clause_tree"),
               ("hybrid", "cursors", "aggs", "rescore", "clauses", "phrases", "fscore", "collapse"),
               "a matcher tree is not built on cursor, hybrid, aggregation, rescore, bool, phrase, function_score or "
               "collapse batches"),
    _BatchKind("collapse", "slg_batch_prepare_collapse", ("sort", "cursors", "collapse"),
               ("hybrid", "aggs", "rescore", "clauses", "phrases", "fscore"),
               "collapse is not built on hybrid, aggregation, rescore, bool, phrase or function_score batches"),
    _BatchKind("fscore", "slg_batch_prepare_fscore", ("sort", "fscore"),
               ("hybrid", "cursors", "aggs", "rescore", "clauses", "phrases"),
               "function_score is not built on cursor, hybrid, aggregation, rescore, bool or phrase batches"),
    _BatchKind("phrases", "slg_batch_prepare_phrase", ("sort", "clauses", "phrases"),
               ("hybrid", "cursors", "aggs", "rescore"),
               "phrases are not built on cursor, hybrid, aggregation or rescore batches"),
    _BatchKind("clauses", "slg_batch_prepare_bool", ("sort", "clauses"), ("hybrid", "cursors", "aggs", "rescore"),
               "boolean clauses are not built on cursor, hybrid, aggregation or rescore batches"),
    _BatchKind("rescore", "slg_batch_prepare_rescore", ("rescore",), ("hybrid", "cursors", "sort", "aggs"),
               "rescore is not built on sorted, cursor, hybrid or aggregation batches"),
    _BatchKind("aggs", "slg_batch_prepare_aggs", ("sort", "agg_spec"), ("hybrid", "cursors"),
               "aggregations are not built on cursor or hybrid batches"),
    _BatchKind("hybrid", "slg_batch_prepare_hybrid", ()),
    _BatchKind("cursors", "slg_batch_prepare_after", ("sort", "cursors")),
    _BatchKind("sort", "slg_batch_prepare_sorted", ("sort",)),
    _BatchKind(None, "slg_batch_prepare_plans", ()),
)


class PreparedBatch:
    """A planned query batch with device-resident descriptors and work buffers."""

    def __init__(self, index: GpuIndex, q_offsets, q_terms, q_weights, k: int, strategy: int,
                 q_filter=None, q_leaf=None, q_plan=None, q_tie=None, q_nleaves=None,
                 q_leaf_offsets=None, leaf_group=None, q_group_offsets=None, group_plan=None,
                 group_tie=None, q_node_offsets=None, node_kind=None, node_tie=None, node_parent=None,
                 q_min_match=None, sort=None, cursors=None, hybrid=False, aggs=None, rescore=None, clauses=None,
                 phrases=None, fscore=None, collapse=None, clause_tree=None, script=None, script_order="outer",
                 top_hits=None, composite=None, term_buckets=None, request=False):
        self.index = index
        self._lib = index._lib
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.uint32)
        q_terms = np.ascontiguousarray(q_terms, dtype=np.uint32)
        q_weights = np.ascontiguousarray(q_weights, dtype=np.float32)
        self.nq = len(q_offsets) - 1
        self.k = k
        qf = None if q_filter is None else np.ascontiguousarray(q_filter, dtype=np.int32)
        assert qf is None or len(qf) == self.nq
        ql = None if q_leaf is None else np.ascontiguousarray(q_leaf, dtype=np.uint32)
        qp = None if q_plan is None else np.ascontiguousarray(q_plan, dtype=np.int32)
        qt = None if q_tie is None else np.ascontiguousarray(q_tie, dtype=np.float32)
        qn = None if q_nleaves is None else np.ascontiguousarray(q_nleaves, dtype=np.uint32)
        assert ql is None or len(ql) == len(q_weights)
        assert all(x is None or len(x) == self.nq for x in (qp, qt, qn))
        opt = lambda a: None if a is None else _ptr(a)
        u32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint32)
        qlo, lg, qgo = u32(q_leaf_offsets), u32(leaf_group), u32(q_group_offsets)
        gp = None if group_plan is None else np.ascontiguousarray(group_plan, dtype=np.int32)
        gt = None if group_tie is None else np.ascontiguousarray(group_tie, dtype=np.float32)
        qno, npar = u32(q_node_offsets), u32(node_parent)
        nk = None if node_kind is None else np.ascontiguousarray(node_kind, dtype=np.int32)
        ntie = None if node_tie is None else np.ascontiguousarray(node_tie, dtype=np.float32)
        qmm = u32(q_min_match)
        assert qmm is None or len(qmm) == self.nq
        plans = N.ScorePlans(opt(ql), opt(qp), opt(qt), opt(qn), opt(qlo), opt(lg), opt(qgo), opt(gp), opt(gt),
                             opt(qno), opt(nk), opt(ntie), opt(npar), opt(qmm))
        self.sorted = sort is not None
        self.after = cursors is not None
        self.is_hybrid = bool(hybrid)
        assert not (hybrid and (sort is not None or cursors is not None)), "a hybrid batch takes no sort or cursor"
        self.is_rescore = rescore is not None
        self.is_bool = clauses is not None or phrases is not None
        self.is_phrase = phrases is not None
        self.is_fscore = fscore is not None
        self.is_collapse = collapse is not None
        self.is_bool_tree = clause_tree is not None
        self.is_script = script is not None
        # an aggs.AggPlan carries its N.AggSpec, its N.TopHitsSpec and its composite and significant_terms /
        # rare_terms nodes, the last two as dicts whose "spec" is the N.CompositeSpec / N.TermBucketSpec
        carried = lambda name, own: getattr(aggs, name, None) if own is None else own
        unwrap = lambda x: x["spec"] if isinstance(x, dict) else x
        self.agg_spec = getattr(aggs, "spec", aggs)
        self.top_hits_spec = carried("top_hits", top_hits)
        self.composite_spec = unwrap(carried("composite", composite))
        self.term_bucket_spec = unwrap(carried("term_buckets", term_buckets))
        family = (self.top_hits_spec, self.composite_spec, self.term_bucket_spec)
        # (a plan of top_hits, composite or term bucket roots alone has no aggregation node)
        if any(x is not None for x in family) and self.agg_spec is not None and int(self.agg_spec.n_nodes) == 0:
            self.agg_spec = None
        given = dict(sort=sort, cursors=cursors, hybrid=hybrid or None, aggs=aggs, rescore=rescore, clauses=clauses,
                     phrases=phrases, fscore=fscore, collapse=collapse, clause_tree=clause_tree, script=script,
                     top_hits=family[0], composite=family[1], term_buckets=family[2])
        kinds = [kd for kd in _BATCH_KINDS if kd.arg is None or given[kd.arg] is not None]
        # The library's other prepare calls take no spec of the kind: the refusal is made here with its code.  The
        # specs an AggPlan can carry speak before a kind is chosen, top_hits first; of the rest the chosen kind alone
        # (a compound request goes to the library as it is: slg_batch_prepare_request refuses what is not built)
        for kd in () if request else [x for x in reversed(_BATCH_KINDS[:3]) if x in kinds] or kinds[:1]:
            if any(given[name] is not None for name in kd.refuses):
                raise N.SlgError(N.ERR_UNSUPPORTED, kd.message)
        held = []  # what only the prepare call reads: alive until it has returned

        def pointer(slot):
            if slot == "script_order":
                return int({"outer": N.SCRIPT_OUTER, "inner": N.SCRIPT_INNER}.get(script_order, script_order))
            if slot.endswith("_spec"):
                return _addr(getattr(self, slot))
            if given[slot] is None:
                return None
            if slot == "sort":
                obj = sort_spec(sort)
            elif slot == "cursors":
                assert len(cursors) == self.nq
                obj = (N.SortCursor * max(self.nq, 1))(*[sort_cursor(c, sort) for c in cursors])
            else:
                make, keep = _SPEC_MAKERS[slot]
                made = given[slot] if isinstance(given[slot], tuple) else make(given[slot], self.nq)
                obj = made[0]
                setattr(self, keep, made[1])
                if slot == "collapse":
                    self.collapse_shape = (int(obj.group_limit), int(obj.inner_size))
            held.append(obj)
            return C.addressof(obj)

        if request:
            if hybrid:
                raise N.SlgError(N.ERR_UNSUPPORTED, "a hybrid batch is not a compound request (slg_batch_prepare_hybrid)")
            req = N.Request(C.sizeof(N.Request), self.nq, _ptr(q_offsets), _ptr(q_terms), _ptr(q_weights),
                            C.addressof(plans), opt(qf), k, strategy,
                            *[pointer(slot) for slot in ("sort", "cursors", "clauses", "phrases", "clause_tree", "fscore",
                                                         "script", "script_order")], 0,
                            *[pointer(slot) for slot in ("agg_spec", "top_hits_spec", "composite_spec",
                                                         "term_bucket_spec", "rescore", "collapse")])
            self._h = self._lib.slg_batch_prepare_request(index._h, C.addressof(req))
        else:
            self._h = getattr(self._lib, kinds[0].entry)(
                index._h, self.nq, _ptr(q_offsets), _ptr(q_terms), _ptr(q_weights), C.addressof(plans), opt(qf),
                *[pointer(slot) for slot in kinds[0].own], k, strategy)
        if not self._h:
            raise N.SlgError(N.last_error_code() or N.ERR_INVALID, N.last_error())
        index._batches.add(self)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.slg_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self) -> None:
        N.check(self._lib.slg_batch_run(self._h))

    def matched_counts(self) -> np.ndarray:
        """Accepted docs per query of a sorted batch's last run (total_matches); waits."""
        out = np.zeros(max(self.nq, 1), dtype=np.uint64)
        N.check(self._lib.slg_batch_matched_counts(self._h, _ptr(out)))
        return out[:self.nq]

    def agg_layout(self) -> list:
        """slg_batch_agg_layout: per node dict(parent_rows, rows, first_id, is_stats, offset)."""
        n = int(self.agg_spec.n_nodes)
        lay = (N.AggLayout * n)()
        N.check(self._lib.slg_batch_agg_layout(self._h, lay))
        return [dict(parent_rows=int(x.parent_rows), rows=int(x.rows), first_id=int(x.first_id),
                     is_stats=int(x.is_stats) == 1, is_values=int(x.is_stats) == 2, offset=int(x.offset)) for x in lay]

    def _agg_tables(self):
        """slg_batch_fetch_aggs / _fetch_agg_values into 2-D arrays: (layout, counts, stats, values, composite
        layout or None).  A composite batch's rows hold the composite's cells behind the spec's."""
        from .aggs import STATS_DTYPE
        lay = self.agg_layout() if self.agg_spec is not None else []
        cells = lambda pick: sum(x["parent_rows"] * x["rows"] for x in lay if pick(x))
        cc = cells(lambda x: not x["is_stats"] and not x["is_values"])
        sc, vc = cells(lambda x: x["is_stats"]), cells(lambda x: x["is_values"])
        cl = self.composite_layout() if getattr(self, "composite_spec", None) is not None else None
        if cl is not None:
            cc += cl["size"] + sum(x["parent_rows"] * x["rows"] for x in cl["children"] if not x["is_stats"])
            sc += sum(x["parent_rows"] * x["rows"] for x in cl["children"] if x["is_stats"])
        if getattr(self, "term_bucket_spec", None) is not None:  # (the same for the nodes with children)
            for nd in self.term_buckets_layout()["nodes"]:
                if nd["children"]:
                    cc += nd["size"] + sum(x["parent_rows"] * x["rows"] for x in nd["children"] if not x["is_stats"])
                    sc += sum(x["parent_rows"] * x["rows"] for x in nd["children"] if x["is_stats"])
        counts = np.zeros((max(self.nq, 1), max(cc, 1)), dtype=np.uint64)
        stats = np.zeros((max(self.nq, 1), max(sc, 1)), dtype=STATS_DTYPE)
        values = np.zeros((max(self.nq, 1), max(vc, 1)), dtype=np.uint64)
        N.check(self._lib.slg_batch_fetch_aggs(self._h, _ptr(counts.reshape(-1)[:self.nq * cc]) if cc else None,
                                               _ptr(stats.reshape(-1)[:self.nq * sc]) if sc else None))
        if vc:
            N.check(self._lib.slg_batch_fetch_agg_values(self._h, _ptr(values.reshape(-1)[:self.nq * vc])))
        flat = lambda src, n: src.reshape(-1)[:self.nq * n].reshape(self.nq, n)
        return lay, flat(counts, cc), flat(stats, sc), flat(values, vc), cl

    @staticmethod
    def _cut(x: dict, counts, stats, values) -> np.ndarray:
        src = stats if x["is_stats"] else values if x["is_values"] else counts
        n = x["parent_rows"] * x["rows"]
        return src[:, x["offset"]:x["offset"] + n].reshape(src.shape[0], x["parent_rows"], x["rows"]).copy()

    def aggs(self) -> list:
        """The tables of the last run (slg_batch_fetch_aggs / _fetch_agg_values; waits): per node an array
        [nq, parent_rows, rows], uint64 counts for a bucket node, aggs.STATS_DTYPE records (count, min, max, sum)
        for a stats node, uint64 value cells for a cardinality, percentiles or percentile_ranks node."""
        lay, counts, stats, values, _ = self._agg_tables()
        return [self._cut(x, counts, stats, values) for x in lay]

    def composite_layout(self) -> dict:
        """slg_batch_composite_layout: dict(n_sources, size, key_bits, count_offset, sources = [dict(shift, bits, slots,
        first_id, zero_slot)], children = [as agg_layout's entries])."""
        lay = N.CompositeLayout()
        N.check(self._lib.slg_batch_composite_layout(self._h, C.addressof(lay)))
        return dict(n_sources=int(lay.n_sources), size=int(lay.size), key_bits=int(lay.key_bits),
                    count_offset=int(lay.count_offset),
                    sources=[dict(shift=int(x.shift), bits=int(x.bits), slots=int(x.slots), first_id=int(x.first_id),
                                  zero_slot=int(x.zero_slot)) for x in lay.sources[:int(lay.n_sources)]],
                    children=[dict(parent_rows=int(x.parent_rows), rows=int(x.rows), first_id=int(x.first_id),
                                   is_stats=int(x.is_stats) == 1, is_values=False, offset=int(x.offset))
                              for x in lay.children[:int(lay.n_children)]])

    def set_composite_after(self, lower=None) -> None:
        """slg_batch_set_composite_after: per query the INCLUSIVE lower bound in packed key space of the runs that
        follow (aggs.composite_lower_bound); None: from the start."""
        arr = None if lower is None else np.ascontiguousarray(lower, dtype=np.uint64)
        assert arr is None or len(arr) == self.nq
        N.check(self._lib.slg_batch_set_composite_after(self._h, _ptr(arr) if arr is not None and self.nq else None))

    def composite(self) -> dict:
        """The page of a composite batch's last run (slg_batch_fetch_composite and the composite's cells of
        slg_batch_fetch_aggs; waits): keys [nq, size] uint64 ascending, n_buckets [nq], has_more [nq], counts
        [nq, size], children = per child an array [nq, size, rows] (as aggs()); zeros past n_buckets."""
        _, counts, stats, values, cl = self._agg_tables()
        nq, size = max(self.nq, 1), cl["size"]
        keys = np.zeros((nq, size), dtype=np.uint64)
        nb, more = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
        N.check(self._lib.slg_batch_fetch_composite(self._h, _ptr(keys), _ptr(nb), _ptr(more)))
        c0 = cl["count_offset"]
        return dict(keys=keys[:self.nq], n_buckets=nb[:self.nq], has_more=more[:self.nq],
                    counts=counts[:, c0:c0 + size].copy(),
                    children=[self._cut(x, counts, stats, values) for x in cl["children"]])

    def term_buckets_layout(self) -> dict:
        """slg_batch_term_buckets_layout: dict(rows, nodes = [dict(size, row_offset, count_offset, children = [as
        agg_layout's entries])])."""
        lay = N.TermBucketLayout()
        N.check(self._lib.slg_batch_term_buckets_layout(self._h, C.addressof(lay)))
        return dict(rows=int(lay.rows), nodes=[
            dict(size=int(n.size), row_offset=int(n.row_offset), count_offset=int(n.count_offset),
                 children=[dict(parent_rows=int(x.parent_rows), rows=int(x.rows), first_id=int(x.first_id),
                                is_stats=int(x.is_stats) == 1, is_values=False, offset=int(x.offset))
                           for x in n.children[:int(n.n_children)]])
            for n in lay.nodes[:int(lay.n_nodes)]])

    def term_buckets(self) -> dict:
        """The buckets of a term bucket batch's last run (slg_batch_fetch_term_buckets and the nodes' cells of
        slg_batch_fetch_aggs; waits): nodes = per node dict(ords uint32, doc_counts, bg_counts, score_bits uint64
        [nq, size] in the response's order, scores float64 (the bits viewed), n_buckets [nq], doc_count, bg_count [nq]
        (the node's totals), counts [nq, size] or None, children = per child an array [nq, size, rows] (as aggs()));
        zeros past n_buckets and for what a rare node does not return."""
        lay = self.term_buckets_layout()
        nq, rows, nn = max(self.nq, 1), lay["rows"], len(lay["nodes"])
        ords = np.zeros((nq, rows), dtype=np.uint32)
        dc, bg, sb = (np.zeros((nq, rows), dtype=np.uint64) for _ in range(3))
        nb = np.zeros((nq, nn), dtype=np.uint32)
        ndc, nbg = np.zeros((nq, nn), dtype=np.uint64), np.zeros((nq, nn), dtype=np.uint64)
        N.check(self._lib.slg_batch_fetch_term_buckets(self._h, _ptr(ords), _ptr(dc), _ptr(bg), _ptr(sb), _ptr(nb),
                                                       _ptr(ndc), _ptr(nbg)))
        tables = self._agg_tables() if any(nd["children"] for nd in lay["nodes"]) else None
        nodes = []
        for i, nd in enumerate(lay["nodes"]):
            r0, r1 = nd["row_offset"], nd["row_offset"] + nd["size"]
            cut = lambda a: a[:self.nq, r0:r1].copy()
            out = dict(ords=cut(ords), doc_counts=cut(dc), bg_counts=cut(bg), score_bits=cut(sb),
                       scores=cut(sb).view(np.float64), n_buckets=nb[:self.nq, i].copy(),
                       doc_count=ndc[:self.nq, i].copy(), bg_count=nbg[:self.nq, i].copy(), counts=None, children=[])
            if nd["children"]:
                _, counts, stats, values, _ = tables
                c0 = nd["count_offset"]
                out["counts"] = counts[:, c0:c0 + nd["size"]].copy()
                out["children"] = [self._cut(x, counts, stats, values) for x in nd["children"]]
            nodes.append(out)
        return dict(nodes=nodes)

    def top_hits_layout(self) -> list:
        """slg_batch_top_hits_layout: per top_hits node dict(lists, size, list_offset, hit_offset)."""
        n = int(self.top_hits_spec.n_nodes)
        lay = (N.TopHitsLayout * n)()
        N.check(self._lib.slg_batch_top_hits_layout(self._h, lay))
        return [dict(lists=int(x.lists), size=int(x.size), list_offset=int(x.list_offset),
                     hit_offset=int(x.hit_offset)) for x in lay]

    def top_hits(self) -> dict:
        """The lists of a top_hits batch's last run (slg_batch_fetch_top_hits; waits): status [nq] (1: the query's
        bucket runs did not fit max_entries, its lists are all zero: the CPU path), and nodes = per top_hits node
        dict(doc, seg, score [nq, lists, size], count [nq, lists]); zeros past the counts."""
        lay = self.top_hits_layout()
        hc = sum(x["lists"] * x["size"] for x in lay)
        lc = sum(x["lists"] for x in lay)
        nq = max(self.nq, 1)
        doc, seg = np.zeros((nq, hc), dtype=np.uint32), np.zeros((nq, hc), dtype=np.uint32)
        score, count = np.zeros((nq, hc), dtype=np.float32), np.zeros((nq, lc), dtype=np.uint32)
        status = np.zeros(nq, dtype=np.uint32)
        N.check(self._lib.slg_batch_fetch_top_hits(self._h, _ptr(doc), _ptr(seg), _ptr(score), _ptr(count), _ptr(status)))
        nodes = []
        for x in lay:
            h0, h1 = x["hit_offset"], x["hit_offset"] + x["lists"] * x["size"]
            cut = lambda a: a[:self.nq, h0:h1].reshape(self.nq, x["lists"], x["size"]).copy()
            nodes.append(dict(doc=cut(doc), seg=cut(seg), score=cut(score),
                              count=count[:self.nq, x["list_offset"]:x["list_offset"] + x["lists"]].copy()))
        return dict(status=status[:self.nq], nodes=nodes)

    def rescore_details(self):
        """Per row of a rescore batch's last run (slg_batch_fetch_rescore; waits): (first_score [nq, k], the
        first-pass score; rescore_score [nq, k], 0.0 where the row was not rescored; rescored [nq, k], 1 where
        it was)."""
        first = np.zeros((self.nq, self.k), dtype=np.float32)
        rsc = np.zeros((self.nq, self.k), dtype=np.float32)
        flag = np.zeros((self.nq, self.k), dtype=np.uint32)
        N.check(self._lib.slg_batch_fetch_rescore(self._h, _ptr(first), _ptr(rsc), _ptr(flag)))
        return first, rsc, flag

    def collapse_groups(self) -> dict:
        """The collapse arrays of a collapse batch's last run (slg_batch_fetch_collapse; waits): n_groups,
        total_groups, status [nq]; group_row, group_ord, group_size, group_doc, group_seg, group_score, inner_count
        [nq, G]; inner_row, inner_doc, inner_seg, inner_score [nq, G, S] (G = group_limit, S = inner_size).  Zeros
        past the counts; a query with status 1 (a row with several values: the request fails) has zeros only."""
        G, S = self.collapse_shape
        names = [("n_groups", ()), ("total_groups", ()), ("status", ()), ("group_row", (G,)), ("group_ord", (G,)),
                 ("group_size", (G,)), ("group_doc", (G,)), ("group_seg", (G,)), ("group_score", (G,)),
                 ("inner_count", (G,)), ("inner_row", (G, S)), ("inner_doc", (G, S)), ("inner_seg", (G, S)),
                 ("inner_score", (G, S))]
        out = {n: np.zeros((self.nq,) + shape, dtype=np.float32 if n.endswith("score") else np.uint32)
               for n, shape in names}
        N.check(self._lib.slg_batch_fetch_collapse(self._h, *[_ptr(out[n]) if out[n].size else None for n, _ in names]))
        return out

    def cursor_seen(self) -> np.ndarray:
        """Per query of a cursor batch's last run: 1 if an accepted doc had the cursor's key (or the query has
        no cursor), 0 for a stale cursor (saw_cursor); waits."""
        out = np.zeros(max(self.nq, 1), dtype=np.uint8)
        N.check(self._lib.slg_batch_cursor_seen(self._h, _ptr(out)))
        return out[:self.nq]

    def run_sharded(self, group: "ShardGroup", fetch: bool = True, seq: Optional[int] = None):
        """slg_batch_run_sharded: this rank's segments, ONE ncclAllGather of the result blocks,
        device merge.  fetch=True -> merged (doc, seg, score, count) host arrays (waits);
        fetch=False -> None, the merged block stays on the device (sharded_device_results).
        seq: slg_batch_run_sharded_seq — the run's number in the group's order of collectives."""
        if not fetch:
            if seq is None:
                N.check(self._lib.slg_batch_run_sharded(self._h, group._h, None, None, None, None))
            else:
                N.check(self._lib.slg_batch_run_sharded_seq(self._h, group._h, int(seq), None, None, None, None))
            return None
        nq, k = self.nq, self.k
        out_doc = np.zeros((nq, k), dtype=np.uint32)
        out_seg = np.zeros((nq, k), dtype=np.uint32)
        out_score = np.zeros((nq, k), dtype=np.float32)
        out_count = np.zeros(nq, dtype=np.uint32)
        N.check(self._lib.slg_batch_run_sharded(self._h, group._h, _ptr(out_doc), _ptr(out_seg),
                                                _ptr(out_score), _ptr(out_count)))
        return out_doc, out_seg, out_score, out_count

    def fetch_sharded(self):
        """Waits for run_sharded(fetch=False) -> merged (doc, seg, score, count) host arrays."""
        nq, k = self.nq, self.k
        out_doc = np.zeros((nq, k), dtype=np.uint32)
        out_seg = np.zeros((nq, k), dtype=np.uint32)
        out_score = np.zeros((nq, k), dtype=np.float32)
        out_count = np.zeros(nq, dtype=np.uint32)
        N.check(self._lib.slg_batch_fetch_sharded(self._h, _ptr(out_doc), _ptr(out_seg), _ptr(out_score),
                                                  _ptr(out_count)))
        return out_doc, out_seg, out_score, out_count

    def sharded_device_results(self):
        """-> (d_doc, d_seg, d_score, d_count) raw device addresses of the merged top-k."""
        ptrs = [C.c_void_p() for _ in range(4)]
        N.check(self._lib.slg_batch_sharded_device_results(self._h, *[C.addressof(p) for p in ptrs]))
        return tuple(p.value for p in ptrs)

    def set_stream(self, hip_stream) -> None:
        """Run this batch on its own hipStream_t so several batches can be in flight at once
        (None: back to the index stream)."""
        h = C.c_void_p(-1) if hip_stream is None else C.c_void_p(int(hip_stream) or None)
        N.check(self._lib.slg_batch_set_stream(self._h, h))

    def rerank_device(self, n_clauses, d_qvecs, d_alpha, d_boost, k_out, d_out_doc, d_out_seg, d_out_score,
                      d_out_vec, d_out_count) -> None:
        """slg_batch_rerank_device: rerank this batch's own device results on the batch's stream."""
        N.check(self._lib.slg_batch_rerank_device(self._h, n_clauses, d_qvecs, d_alpha, d_boost, k_out, d_out_doc,
                                                  d_out_seg, d_out_score, d_out_vec, d_out_count))

    def hybrid_device(self, clause_field, d_qvecs, d_alpha, d_boost, cand_size, k_out, d_out_doc, d_out_seg,
                      d_out_score, d_out_vec, d_out_count, d_out_total) -> None:
        """slg_batch_hybrid_device: the vector side of a hybrid batch (prepare(..., hybrid=True)) after run(),
        on the batch's stream; device addresses (ints), clause_field a host array, d_boost may be None."""
        cf = np.ascontiguousarray(clause_field, dtype=np.uint32)
        N.check(self._lib.slg_batch_hybrid_device(self._h, len(cf), _ptr(cf), d_qvecs, d_alpha, d_boost,
                                                  int(cand_size), int(k_out), d_out_doc, d_out_seg, d_out_score,
                                                  d_out_vec, d_out_count, d_out_total))

    def hybrid(self, clause_field, qvecs, alpha, cand_size: int, k_out: int, boost=None):
        """run() + hybrid_device() with host arrays (staged through torch tensors on the index's device);
        waits.  -> (doc, seg, score, vec_score) [nq, k_out], count [nq], total [nq]."""
        import torch
        nq, nc = self.nq, len(clause_field)
        dev = torch.device("cuda", self.index.device)
        up = lambda a: None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)  # (a writable copy)
        t_q = up(np.ascontiguousarray(qvecs, dtype=np.float32).reshape(nq, -1))
        t_a, t_b = up(_f32(alpha, (nq, nc))), up(_f32(boost, (nq, nc)))
        o_doc = torch.zeros((nq, k_out), dtype=torch.int32, device=dev)
        o_seg = torch.zeros_like(o_doc)
        o_score = torch.zeros((nq, k_out), dtype=torch.float32, device=dev)
        o_vec = torch.zeros_like(o_score)
        o_cnt = torch.zeros(max(nq, 1), dtype=torch.int32, device=dev)
        o_tot = torch.zeros(max(nq, 1), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        self.run()
        ptr = lambda t: None if t is None else t.data_ptr()
        self.hybrid_device(clause_field, ptr(t_q), ptr(t_a), ptr(t_b), cand_size, k_out, ptr(o_doc), ptr(o_seg),
                           ptr(o_score), ptr(o_vec), ptr(o_cnt), ptr(o_tot))
        self.sync()
        return (o_doc.cpu().numpy().view(np.uint32), o_seg.cpu().numpy().view(np.uint32), o_score.cpu().numpy(),
                o_vec.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint32)[:nq],
                o_tot.cpu().numpy().view(np.uint64)[:nq])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self) -> None:
        N.check(self._lib.slg_batch_sync(self._h))

    def info(self):
        npost, nsl, nbytes = C.c_uint64(), C.c_uint32(), C.c_uint64()
        N.check(self._lib.slg_batch_info(self._h, C.addressof(npost), C.addressof(nsl),
                                         C.addressof(nbytes)))
        out = {"n_postings": npost.value, "n_slices": nsl.value, "algorithmic_bytes": nbytes.value}
        if getattr(self, "is_fscore", False):  # which fscore_kernel runs: None (nothing is launched), "lean", "full"
            variant, work = C.c_uint32(), C.c_uint32()
            N.check(self._lib.slg_batch_fscore_info(self._h, C.addressof(variant), C.addressof(work)))
            out["fscore_kernel"] = (None, "lean", "full")[variant.value]
            out["fscore_queries"] = work.value
        if getattr(self, "is_script", False):
            work, depth = C.c_uint32(), C.c_uint32()
            N.check(self._lib.slg_batch_script_info(self._h, C.addressof(work), C.addressof(depth)))
            out["script_queries"] = work.value
            out["script_max_depth"] = depth.value
        return out

    def skip_counts(self):
        """-> (postings of pruning-classified lists the plan covered, those never loaded) of the
        last run (block skipping, query/wand.rs:205-265)."""
        probed, skipped = C.c_uint64(), C.c_uint64()
        N.check(self._lib.slg_batch_skip_counts(self._h, C.addressof(probed), C.addressof(skipped)))
        return probed.value, skipped.value

    def device_results(self):
        """-> (d_doc, d_seg, d_score, d_count) raw device addresses."""
        ptrs = [C.c_void_p() for _ in range(4)]
        N.check(self._lib.slg_batch_device_results(self._h, *[C.addressof(p) for p in ptrs]))
        return tuple(p.value for p in ptrs)

    def device_result_block(self):
        """-> (address, n_bytes) of the contiguous doc|seg|score|count block."""
        ptr, nb = C.c_void_p(), C.c_uint64()
        N.check(self._lib.slg_batch_device_result_block(self._h, C.addressof(ptr), C.addressof(nb)))
        return ptr.value, nb.value

    def fetch(self, want_stats: bool = False):
        nq, k = self.nq, self.k
        out_doc = np.zeros((nq, k), dtype=np.uint32)
        out_seg = np.zeros((nq, k), dtype=np.uint32)
        out_score = np.zeros((nq, k), dtype=np.float32)
        out_count = np.zeros(nq, dtype=np.uint32)
        stats = (N.Stats * max(nq, 1))() if want_stats else None
        N.check(self._lib.slg_batch_fetch(self._h, _ptr(out_doc), _ptr(out_seg), _ptr(out_score),
                                          _ptr(out_count),
                                          None if stats is None else C.addressof(stats)))
        if want_stats:
            return out_doc, out_seg, out_score, out_count, stats
        return out_doc, out_seg, out_score, out_count

    def highlight(self, specs):
        """slg_batch_highlight: the batch's own device rows highlighted under specs[q] = [highlight_spec() dicts],
        against the index state the batch was prepared on -> result[q][row][spec] = (status, [fragment bytes]) for
        the rows in front of count[q] (highlight.py; the counts that shape the result come from fetch()).  The
        batch must have run."""
        from .highlight import highlight_batch
        return highlight_batch(self._lib, self._h, self.fetch()[3], specs)

    def explain(self, rows: int) -> dict:
        """slg_batch_explain: the first min(rows, count[q]) rows of every query explained, against the index state
        the batch was prepared on -> the raw arrays, by the names of slg_explain_out: base_score, final_score,
        n_functions [nq, rows]; fn_type, fn_field, fn_value [nq, rows, MAX_EXPLAIN_FUNCS]; a rescore batch also
        rescored, rescore_score, combined_score [nq, rows].  Rows at or beyond a query's count are zero.  The batch
        must have run; explain.shape() turns the arrays into the reference's JSON form."""
        nq, nf = self.nq, N.MAX_EXPLAIN_FUNCS
        r = max(int(rows), 1)  # (rows 0 is refused by the library: the arrays only have to exist)
        out = dict(base_score=np.zeros((nq, r), np.float32), final_score=np.zeros((nq, r), np.float32),
                   n_functions=np.zeros((nq, r), np.uint32), fn_type=np.zeros((nq, r, nf), np.uint32),
                   fn_field=np.zeros((nq, r, nf), np.int32), fn_value=np.zeros((nq, r, nf), np.float32))
        if getattr(self, "is_rescore", False):  # (a ScanBatch has no such kind: the library refuses it by name)
            out.update(rescored=np.zeros((nq, r), np.uint32), rescore_score=np.zeros((nq, r), np.float32),
                       combined_score=np.zeros((nq, r), np.float32))
        arg = N.ExplainOut(**{name: a.ctypes.data for name, a in out.items()})
        N.check(self._lib.slg_batch_explain(self._h, int(rows), C.addressof(arg)))
        return out


class ScanBatch(PreparedBatch):
    """A planned batch of unscored root queries — match_all, constant_score, rank_feature — whose candidates come
    from a scan over the segments' docs (slg_batch_prepare_scan).  Everything behind prepare is PreparedBatch's:
    run, fetch, matched_counts (every scan batch has them), agg_layout, aggs, device_results, set_stream, sync."""

    def __init__(self, index: GpuIndex, queries, k: int, sort=None, aggs=None, q_filter=None):
        from .scan import scan_spec
        self.index = index
        self._lib = index._lib
        sspec, self._scan_keep = queries if isinstance(queries, tuple) else scan_spec(queries)
        self.nq = len(self._scan_keep["q_kind"])
        self.k = k
        qf = None if q_filter is None else np.ascontiguousarray(q_filter, dtype=np.int32)
        assert qf is None or len(qf) == self.nq
        self.sorted = sort is not None
        self.after = False
        self.is_hybrid = False
        self.is_scan = True
        if getattr(aggs, "top_hits", None) is not None:
            # (slg_batch_prepare_scan takes no top_hits spec: refused here with the library's code, nothing dropped)
            raise N.SlgError(N.ERR_UNSUPPORTED, "top_hits is not built on scan batches")
        if getattr(aggs, "composite", None) is not None:  # (the same for a composite)
            raise N.SlgError(N.ERR_UNSUPPORTED, "composite is not built on scan batches")
        if getattr(aggs, "term_buckets", None) is not None:  # (and for significant_terms / rare_terms)
            raise N.SlgError(N.ERR_UNSUPPORTED, "significant_terms and rare_terms are not built on scan batches")
        self.composite_spec = None
        self.term_bucket_spec = None
        self.agg_spec = getattr(aggs, "spec", aggs)  # (an aggs.AggPlan carries its N.AggSpec)
        spec = None if sort is None else sort_spec(sort)
        self._h = self._lib.slg_batch_prepare_scan(
            index._h, self.nq, C.addressof(sspec), _ptr(qf), None if spec is None else C.addressof(spec),
            None if self.agg_spec is None else C.addressof(self.agg_spec), k)
        if not self._h:
            raise N.SlgError(N.last_error_code() or N.ERR_INVALID, N.last_error())
        index._batches.add(self)

    def info(self):
        out = super().info()
        variant, slices, docs = C.c_uint32(), C.c_uint32(), C.c_uint32()
        N.check(self._lib.slg_batch_scan_info(self._h, C.addressof(variant), C.addressof(slices), C.addressof(docs)))
        out["scan_kernel"] = (None, "lean", "full")[variant.value]  # None: the batch has no slice
        out["n_slices"] = slices.value
        out["scan_slice_docs"] = docs.value
        return out
