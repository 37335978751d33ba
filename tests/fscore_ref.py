"""Numpy restatement of function_score at the root of the score tree (evaluate_compiled_score, api/reader.rs:491-548;
query/score_functions.rs) in the flat form of slg_batch_prepare_fscore, over the oracle.

Per candidate doc with first-pass score `base` (f32):
  every function, in request order, gives a value (f32) or none.  A function with a filter gives none to a doc the
  filter rejects.
    weight              -> weight
    field_value_factor  -> raw = the doc's FIRST value of the column (an i64 value `as f64`), or `missing`;
                           scaled = raw * f64(f32 factor); not finite: none; m = modifier(scaled): none x, log
                           x <= 0 ? 0 : ln x, log1p x <= -1 ? 0 : log1p x, log2p x <= -1 ? 0 : log2(x + 1), sqrt
                           x < 0 ? 0 : sqrt x, reciprocal x == 0 ? 0 : 1 / x; not finite: none; the value is f32(m)
    decay               -> no value of the column: none; distance = |v - origin| - offset, norm = max(distance, 0) /
                           scale; exp pow(decay, norm), gauss pow(decay, norm * norm), linear max((1 - norm) *
                           (1 - decay) + decay, 0); not finite: none; the value is f32 of it
  all f64, one operation at a time.  fs = the present values folded left to right in f32 by score_mode (sum,
  multiply, max, min; avg: the sum over their number; max / min are fmax / fmin: a NaN operand loses).  eff = base,
  but 1.0 when |base| <= f32 epsilon and a value is present.  combined = eff without a value, else boost_mode(eff,
  fs): multiply, sum, replace, max, min.  Then combined = fmin(combined, max_boost) if given; the doc is DROPPED if
  min_score is given and combined < min_score; then combined *= boost.  A query whose entry is None is untouched.

reference(): the oracle's exhaustive result (k = number of docs) over tombstone-free copies of the segments gives
every doc of the scored lists with its exact score (idf uses Segment.docs, a separate field).  evaluate() rewrites
and drops; what is left is `scored_docs` (slg_stats counts tombstoned and filtered docs too, and the bitmap of a
registered filter rejects tombstoned docs, so a function under a filter gives them no value); the live docs among
them that pass the query's own filter are `matched`, ranked by f32 total order descending, then segment, then doc.

The only operations not correctly rounded are ln, log1p, log2 and pow.  Their f64 result y is then rounded to f32;
safe(y) tells that y is further than 2^-40 * |y| from the midpoint of the two neighbouring f32 values — thousands of
f64 ulps, far above the error of numpy's, Rust's or a GPU's functions — so every implementation rounds it to the
same f32.  unsafe_draws() lists the (field, segment, doc) whose value some transcendental function of a spec turns
into an unsafe y; a test world replaces those values and asserts that none is left before it compares bit for bit."""
import copy

import numpy as np

F32, F64 = np.float32, np.float64
EPS = F32(np.finfo(np.float32).eps)
TRANSCENDENTAL_MODIFIERS = ("log", "log1p", "log2p")


def safe(y):
    """y (f64 array) -> bool array: rounding y to f32 cannot depend on the last bits of y"""
    y = np.asarray(y, F64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = y.astype(F32)
        up, down = np.nextafter(f, F32(np.inf)), np.nextafter(f, F32(-np.inf))
        lo = np.where(f.astype(F64) <= y, f, down).astype(F64)
        hi = np.where(f.astype(F64) <= y, up, f).astype(F64)
        mid = lo / 2 + hi / 2
        ok = np.abs(y - mid) > np.abs(y) * 2.0 ** -40
    return ok | ~np.isfinite(y) | ~np.isfinite(mid)


class Columns:
    """fields: {id: (per segment a list of n_docs value lists or None, dtype)} as GpuIndex.add_agg_field takes them;
    filters: {id: per segment a bool mask or None}.  first(field, seg) -> (f64 first value per doc, has-a-value)"""

    def __init__(self, segs, fields=None, filters=None):
        self.segs, self.fields, self.filters = segs, fields or {}, filters or {}
        self._first = {}

    def first(self, field, s):
        if (field, s) not in self._first:
            per_seg, dt = self.fields[field]
            n = self.segs[s].n_docs
            val, has = np.zeros(n, F64), np.zeros(n, bool)
            if per_seg[s] is not None:
                for d, vs in enumerate(per_seg[s]):
                    if len(vs):
                        val[d], has[d] = F64(np.asarray(vs, dt)[0]), True  # (i64 -> `as f64`)
            self._first[(field, s)] = (val, has)
        return self._first[(field, s)]

    def filter_passes(self, fid, s, docs):
        ok = np.ones(len(docs), bool)
        if fid is not None and fid >= 0:
            m = self.filters[fid][s]
            if m is not None:
                ok &= np.asarray(m, bool)[docs]
            dead = self.segs[s].deleted
            if dead is not None:  # (the registered bitmap is deleted | ~filter)
                ok &= ~np.unpackbits(np.asarray(dead, np.uint8), bitorder="little")[docs].astype(bool)
        return ok


def modifier(x, name):
    x = np.asarray(x, F64)
    with np.errstate(all="ignore"):
        if name == "none":
            return x.copy()
        if name == "log":
            return np.where(x <= 0.0, 0.0, np.log(np.where(x <= 0.0, 1.0, x)))
        if name == "log1p":
            return np.where(x <= -1.0, 0.0, np.log1p(np.where(x <= -1.0, 0.0, x)))
        if name == "log2p":
            return np.where(x <= -1.0, 0.0, np.log2(np.where(x <= -1.0, 0.0, x) + 1.0))
        if name == "sqrt":
            return np.where(x < 0.0, 0.0, np.sqrt(np.where(x < 0.0, 0.0, x)))
        if name == "reciprocal":
            return np.where(x == 0.0, 0.0, 1.0 / np.where(x == 0.0, 1.0, x))
    raise ValueError(name)


def function_value(fn, cols, s, docs):
    """-> (value f32, present bool, y f64 = the f64 result a transcendental function gave or None)"""
    n = len(docs)
    has = cols.filter_passes(fn.get("filter", -1), s, docs)
    kind = fn["kind"]
    if kind == "weight":
        return np.full(n, F32(fn["weight"])), has, None
    val, valued = cols.first(fn["field"], s)
    val, valued = val[docs], valued[docs]
    y = None
    with np.errstate(all="ignore"):
        if kind == "field_value_factor":
            raw = np.where(valued, val, F64(fn.get("missing", 0.0)))
            scaled = raw * F64(F32(fn.get("factor", 1.0)))
            m = modifier(scaled, fn.get("modifier", "none"))
            if fn.get("modifier", "none") in TRANSCENDENTAL_MODIFIERS:
                y = m
            has = has & np.isfinite(scaled) & np.isfinite(m)
        elif kind == "decay":
            origin, scale = F64(fn["origin"]), F64(fn["scale"])
            offset, decay = F64(fn.get("offset", 0.0)), F64(fn.get("decay", 0.5))
            distance = np.abs(val - origin) - offset
            norm = np.fmax(distance, 0.0) / scale
            shape = fn.get("function", "exp")
            if shape == "linear":
                m = np.fmax((1.0 - norm) * (1.0 - decay) + decay, 0.0)
            else:
                m = np.power(decay, norm * norm if shape == "gauss" else norm)
                y = m
            has = has & valued & np.isfinite(m)
        else:
            raise ValueError(kind)
        return m.astype(F32), has, y


def evaluate(fsq, cols, s, docs, base):
    """one query's function_score over the docs of segment s with first-pass scores base -> (score f32, kept)"""
    base = np.asarray(base, F32)
    if fsq is None:
        return base.copy(), np.ones(len(base), bool)
    n = len(base)
    fs, present = np.zeros(n, F32), np.zeros(n, np.int64)
    mode = fsq.get("score_mode", "multiply")
    with np.errstate(all="ignore"):
        for fn in fsq.get("functions", ()):
            val, has, _ = function_value(fn, cols, s, docs)
            if mode == "multiply":
                nxt = fs * val
            elif mode == "max":
                nxt = np.fmax(fs, val)
            elif mode == "min":
                nxt = np.fmin(fs, val)
            else:
                nxt = fs + val
            fs = np.where(has, np.where(present == 0, val, nxt), fs).astype(F32)
            present += has
        any_ = present > 0
        eff = np.where(any_ & (np.abs(base) <= EPS), F32(1.0), base).astype(F32)
        if mode == "avg":
            fs = np.where(any_, fs / np.maximum(present, 1).astype(F32), fs).astype(F32)
        bm = fsq.get("boost_mode", "multiply")
        boosted = {"multiply": eff * fs, "sum": eff + fs, "replace": fs, "max": np.fmax(eff, fs),
                   "min": np.fmin(eff, fs)}[bm].astype(F32)
        combined = np.where(any_, boosted, eff).astype(F32)
        if fsq.get("max_boost") is not None:
            combined = np.fmin(combined, F32(fsq["max_boost"])).astype(F32)
        kept = np.ones(n, bool)
        if fsq.get("min_score") is not None:
            kept = ~(combined < F32(fsq["min_score"]))
        combined = (combined * F32(fsq.get("boost", 1.0))).astype(F32)
    return combined, kept


def unsafe_draws(functions, cols):
    """{(field, segment, doc)} whose value a transcendental function of the spec turns into an unsafe y"""
    out = set()
    for fsq in functions:
        for fn in (fsq or {}).get("functions", ()):
            if fn["kind"] == "weight":
                continue
            for s, seg in enumerate(cols.segs):
                docs = np.arange(seg.n_docs)
                _, _, y = function_value(dict(fn, filter=-1), cols, s, docs)
                if y is not None:
                    out |= {(fn["field"], s, int(d)) for d in docs[~safe(y)]}
    return out


def total_key(x):
    """f32 -> int64 that orders as f32::total_cmp"""
    b = np.asarray(x, F32).view(np.int32).astype(np.int64)
    return b ^ ((b >> 31) & 0x7FFFFFFF)


def all_candidates(oracle, segs, q_offsets, q_terms, q_weights, **plans):
    """every doc of the scored lists with its exact first-pass score, tombstoned ones included: the oracle's
    exhaustive run over tombstone-free copies -> (doc, seg, score, count)"""
    bare = []
    for s in segs:
        c = copy.copy(s)
        c.deleted = None
        bare.append(c)
    k_all = sum(s.n_docs for s in segs)
    return oracle.search_batch(bare, q_offsets, q_terms, q_weights, k_all, strategy=oracle.BM25, **plans)


def apply(cands, segs, functions, cols, k, q_filter=None):
    """all_candidates() under one function_score per query -> (doc, seg, score, count) at k, scored_docs, matched,
    and per query the ranked survivors [(seg, doc, score)] (for a field sort on top)"""
    doc, seg, score, count = cands
    nq = len(count)
    out = (np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.uint32), np.zeros((nq, k), F32), np.zeros(nq, np.uint32))
    scored, matched, rows = np.zeros(nq, np.uint64), np.zeros(nq, np.uint64), []
    for q in range(nq):
        n = int(count[q])
        d, sg, sc = doc[q, :n].astype(np.int64), seg[q, :n].astype(np.int64), score[q, :n]
        new, kept, live = np.zeros(n, F32), np.zeros(n, bool), np.ones(n, bool)
        for s, sobj in enumerate(segs):
            at = np.nonzero(sg == s)[0]
            new[at], kept[at] = evaluate(functions[q], cols, s, d[at], sc[at])
            if sobj.deleted is not None:
                live[at] &= ~np.unpackbits(np.asarray(sobj.deleted, np.uint8), bitorder="little")[d[at]].astype(bool)
            f = -1 if q_filter is None else int(q_filter[q])
            if f >= 0 and cols.filters[f][s] is not None:
                live[at] &= np.asarray(cols.filters[f][s], bool)[d[at]]
        scored[q] = int(kept.sum())
        at = np.nonzero(kept & live)[0]
        matched[q] = len(at)
        order = at[np.lexsort((d[at], sg[at], -total_key(new[at])))]
        rows.append([(int(sg[i]), int(d[i]), new[i]) for i in order])
        m = min(k, len(order))
        out[0][q, :m], out[1][q, :m], out[2][q, :m], out[3][q] = d[order[:m]], sg[order[:m]], new[order[:m]], m
    return out, scored, matched, rows
