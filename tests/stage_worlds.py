"""The worlds of tests/test_gpu_stage_edges.py: small segments that put the staging kernels of slg_stage.hpp
(impacts, champions, the bitmap / range / term filters) on their value, list-length and word edges.
tests/test_stage_worlds.py asserts on the CPU that every edge is present."""
from __future__ import annotations

import copy

import numpy as np

from searchlite_amd.segment import Segment

NO_TERM = 0xFFFFFFFF
F32 = np.float32

# ---- V: values -----------------------------------------------------------------------------------------
V_DOCS = 203
V_PARAMS = ((0.9, 0.4), (0.0, 0.75), (1.2, 0.0), (1.2, 1.0), (2.0, 0.75))  # (k1, b) of the five segments
V_TFS = (0, 1, 2, 2 ** 24, 2 ** 24 + 1, 2 ** 32 - 1, 3, 7)
V_AVGDL = (7.5, 0.25, 3.0, 0.0, 1e30)
V_LENS0 = (0.0, -3.0, 0.5, 1.0, 1e30, 3e38, 4.0, 7.0, 12.0, 20.0, 7.5)
V_FULL_DF = V_DOCS  # the df of the lists of every doc


def v_layout():
    """-> (term_offsets, doc_ids, tfs, term_field, names): per field a list of one doc, one of every doc, one of
    every third doc and one of two docs; an empty list as the first, a middle and the last term."""
    lists, fields, names = [], [], []
    empty = np.zeros(0, dtype=np.uint32)

    def add(name, f, docs):
        names.append(name)
        fields.append(f)
        lists.append(np.asarray(docs, dtype=np.uint32))

    add("empty_first", 0, empty)
    for f in range(5):
        add(f"one{f}", f, [(37 * (f + 1)) % V_DOCS])
        add(f"all{f}", f, np.arange(V_DOCS))
        add(f"third{f}", f, np.arange(f % 3, V_DOCS, 3))
        add(f"ends{f}", f, [0, V_DOCS - 1])
        if f == 2:
            add("empty_mid", 2, empty)
    add("empty_last", 4, empty)
    offs = np.zeros(len(lists) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in lists])
    docs = np.concatenate(lists).astype(np.uint32)
    # every tf value meets every doc-length value: doc % 11 picks the length of field 0, doc // 11 (and the list) the tf
    term = np.repeat(np.arange(len(lists)), [len(x) for x in lists])
    tfs = np.array(V_TFS, dtype=np.uint64)[(docs.astype(np.int64) // len(V_LENS0) + term) % len(V_TFS)].astype(np.uint32)
    return offs, docs, tfs, np.array(fields, dtype=np.uint16), names


def v_lengths():
    """the length columns of the five fields (field 2 has none)"""
    d = np.arange(V_DOCS)
    l0 = np.array(V_LENS0, dtype=F32)[d % len(V_LENS0)]
    l1 = np.zeros(V_DOCS, dtype=F32)  # mostly missing: a missing length counts as max(0.25, 1) = 1
    l1[d % 7 == 3] = 0.25
    l1[d % 11 == 5] = 2.0
    l1[40:56] = 5e37  # / 0.25: a denominator near f32::MAX, an impact below the smallest normal f32
    l3 = np.array([0.0, 2.0, 5.0], dtype=F32)[d % 3]
    l4 = np.array([0.0, 1.0, 3e38, 1e30, 1e29], dtype=F32)[d % 5]
    return [l0, l1, None, l3, l4]


def v_segments():
    """five segments over one posting layout: (k1, b) from V_PARAMS; docs = n_docs, df - 1 of the full lists, 1.0"""
    offs, docs, tfs, tfield, _ = v_layout()
    lens = v_lengths()
    live = (float(V_DOCS), float(V_FULL_DF - 1), 1.0, float(V_DOCS), float(V_FULL_DF - 1))
    return [Segment(n_docs=V_DOCS, term_offsets=offs.copy(), doc_ids=docs.copy(), tfs=tfs.copy(),
                    field_doc_len=[None if a is None else a.copy() for a in lens],
                    field_avgdl=np.array(V_AVGDL, dtype=F32), docs=live[i], k1=k1, b=b, term_field=tfield.copy())
            for i, (k1, b) in enumerate(V_PARAMS)]


def v_queries(n_terms: int):
    """-> (q_offsets, q_terms[., 5], q_weights): n_terms == 1: every non-empty list at weight 1; 3 or 7: windows
    of that many consecutive terms walking over the whole dictionary (the empty lists among them)"""
    offs, _, _, _, names = v_layout()
    df = np.diff(offs.astype(np.int64))
    if n_terms == 1:
        rows = [[t] for t in range(len(names)) if df[t] > 0]
    else:
        rows = [[(t + i) % len(names) for i in range(n_terms)] for t in range(0, len(names), 2)]
    flat = np.array([t for r in rows for t in r], dtype=np.uint32)
    q_offsets = np.zeros(len(rows) + 1, dtype=np.uint32)
    q_offsets[1:] = np.cumsum([len(r) for r in rows])
    return q_offsets, np.repeat(flat[:, None], len(V_PARAMS), axis=1), np.ones(len(flat), dtype=F32)


def v_updates():
    """-> [(deleted bitmap or None, live_docs)] for one segment: tombstones that grow (doc 0 and the last doc among
    them; live_docs of the second step lies below the df of the every-third-doc lists), then no bitmap and another
    live_docs"""
    dead = np.zeros(V_DOCS, dtype=bool)
    dead[[0, V_DOCS - 1, 5, 64, 100]] = True
    first = (np.packbits(dead, bitorder="little"), float(V_DOCS - int(dead.sum())))
    dead = dead.copy()
    dead[np.arange(1, V_DOCS, 4)] = True
    second = (np.packbits(dead, bitorder="little"), 40.0)
    return [first, second, (None, 150.0)]


def with_update(seg, deleted, live_docs):
    s = copy.copy(seg)
    s.deleted = None if deleted is None else np.ascontiguousarray(deleted, dtype=np.uint8)
    s.docs = float(live_docs)
    return s


# ---- C: champions --------------------------------------------------------------------------------------
C_DOCS = 4200
C_DFS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049,
         4160)  # (4160: the only length at which one lane holds 64 postings and more)
C_LAYOUTS = ("desc", "asc", "lane", "equal")
C_LANE = 5  # the lane (posting position % 64) that holds the 64 largest impacts of a "lane" list
C_KS = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024)


def c_segment():
    """One field, one list per (df, layout); term id = C_DFS.index(df) * 4 + C_LAYOUTS.index(layout).  The docs of
    a list are spread over the segment; tf = 1 + rank for the wanted order (a larger tf, a larger impact): impacts
    are distinct within a list, except in "equal" lists (tf 1 everywhere)."""
    # one length, 1000 times the average: the denominator is far above every tf, so a step of tf moves the impact
    # by far more than an ulp and a list's impacts are distinct and ordered as its tfs are
    lens = np.full(C_DOCS, 8000.0, dtype=F32)
    lists, tfl = [], []
    for df in C_DFS:
        docs = (np.arange(df, dtype=np.int64) * C_DOCS // max(df, 1)).astype(np.uint32)  # strictly increasing: df <= C_DOCS
        for layout in C_LAYOUTS:
            pos = np.arange(df)
            if layout == "desc":
                tf = df - pos
            elif layout == "asc":
                tf = 1 + pos
            elif layout == "equal":
                tf = np.ones(df, dtype=np.int64)
            else:  # the 64 largest in one lane, largest first; the others ascending
                tf = np.zeros(df, dtype=np.int64)
                in_lane = pos[pos % 64 == C_LANE][:64]
                rest = np.setdiff1d(pos, in_lane)
                tf[rest] = 1 + np.arange(len(rest))
                tf[in_lane] = df - np.arange(len(in_lane))
            lists.append(docs)
            tfl.append(tf.astype(np.uint32))
    offs = np.zeros(len(lists) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in lists])
    return Segment(n_docs=C_DOCS, term_offsets=offs, doc_ids=np.concatenate(lists).astype(np.uint32),
                   tfs=np.concatenate(tfl).astype(np.uint32), field_doc_len=[lens],
                   field_avgdl=np.array([8.0], dtype=F32), docs=float(C_DOCS), k1=1.2, b=0.75)


def c_term(df: int, layout: str) -> int:
    return C_DFS.index(df) * len(C_LAYOUTS) + C_LAYOUTS.index(layout)


def c_tombstones(seg):
    """-> (bitmap, live_docs): dead are the docs of the 30 largest impacts of the descending list of 2049, of a whole
    lane's postings of the ascending list of 1025, doc 0 and the last doc"""
    dead = np.zeros(C_DOCS, dtype=bool)
    d, _ = seg.postings(c_term(2049, "desc"))
    dead[d[:30]] = True
    d, _ = seg.postings(c_term(1025, "asc"))
    dead[d[7::64]] = True
    dead[[0, C_DOCS - 1]] = True
    return np.packbits(dead, bitorder="little"), float(C_DOCS - int(dead.sum()))


def c_queries(n_terms: int):
    """one-term queries over every non-empty list; 3-term queries over lists of neighbouring dfs and layouts"""
    n = len(C_DFS) * len(C_LAYOUTS)
    if n_terms == 1:
        rows = [[t] for t in range(len(C_LAYOUTS), n)]
    else:
        rows = [[t, (t + 5) % n, (t + 10) % n] for t in range(len(C_LAYOUTS), n, 3)]
    flat = np.array([t for r in rows for t in r], dtype=np.uint32)
    q_offsets = np.zeros(len(rows) + 1, dtype=np.uint32)
    q_offsets[1:] = np.cumsum([len(r) for r in rows])
    return q_offsets, flat[:, None].copy(), np.ones(len(flat), dtype=F32)


# ---- F: the bitmap, range and term filters ---------------------------------------------------------------
F_DOCS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000)
F_LAST_DEAD = (33, 64, 256, 1000)  # segments whose last doc is dead
F_TERM_DFS = (1, 255, 256, 257)    # terms 0..3 (absent from the segments too small for them); term 4: doc 0 and the last doc
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
P53 = 2 ** 53
I64_VALUES = (I64_MIN, I64_MAX, P53 + 1, -(P53 + 1), 0, P53, -P53, 7, -7, I64_MIN + 1, I64_MAX - 1)
F64_LO, F64_HI = -1.5, 2.25        # the bounds whose nextafter neighbours sit in the column
F64_VALUES = (np.nan, np.inf, -np.inf, -0.0, 0.0, F64_LO, np.nextafter(F64_LO, -np.inf), np.nextafter(F64_LO, np.inf),
              F64_HI, np.nextafter(F64_HI, -np.inf), np.nextafter(F64_HI, np.inf), 1.0)


def f_world():
    """-> dict: segs (eleven one-field segments), i64 / f64 (a column per segment), terms (term ids [5, n_segs] with
    NO_TERM where the segment lacks the term)"""
    segs, i64, f64 = [], [], []
    terms = np.full((len(F_TERM_DFS) + 1, len(F_DOCS)), NO_TERM, dtype=np.uint32)
    for s, n in enumerate(F_DOCS):
        lists = []
        for j, df in enumerate(F_TERM_DFS):
            if df <= n and not (df == 1 and n == 31):  # (term 0 is absent from the 31-doc segment as well)
                terms[j, s] = len(lists)
                lists.append(np.arange(n - df, n) if j % 2 else np.arange(df))  # at the front / at the end
        terms[len(F_TERM_DFS), s] = len(lists)
        lists.append(np.unique([0, n - 1]))
        lists.append(np.arange(0, n, 3))  # what the batch's queries score
        offs = np.zeros(len(lists) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(x) for x in lists])
        docs = np.concatenate(lists).astype(np.uint32)
        dead = None
        if n in F_LAST_DEAD:
            bits = np.zeros(n, dtype=bool)
            bits[n - 1] = True
            dead = np.packbits(bits, bitorder="little")
        segs.append(Segment(n_docs=n, term_offsets=offs, doc_ids=docs, tfs=(1 + docs % 3).astype(np.uint32),
                            field_doc_len=[(3 + np.arange(n) % 9).astype(F32)], field_avgdl=np.array([7.0], dtype=F32),
                            docs=float(n - (dead is not None)), k1=0.9, b=0.4, deleted=dead))
        d = np.arange(n)
        i64.append(np.array(I64_VALUES, dtype=np.int64)[(d + s) % len(I64_VALUES)])
        f64.append(np.array(F64_VALUES, dtype=np.float64)[(d + 2 * s) % len(F64_VALUES)])
    return {"segs": segs, "i64": i64, "f64": f64, "terms": terms, "score_term": [s.n_terms - 1 for s in segs]}


def f_masks(kind: str, segs):
    """host bitmaps per segment: None, all false, only doc 0, only the last doc"""
    out = []
    for s in segs:
        m = np.zeros(s.n_docs, dtype=bool)
        if kind == "first":
            m[0] = True
        elif kind == "last":
            m[-1] = True
        out.append(None if kind == "none" else m)
    return out


def f_cases(W):
    """-> [(name, kind, per-segment args)]: kind and args as tests/stage_ref.filter_pass takes them"""
    n_segs = len(W["segs"])
    cases = [("bitmap " + k, "bitmap", f_masks(k, W["segs"])) for k in ("none", "empty", "first", "last")]
    i64_ranges = {"lo == hi": (7, 7), "lo > hi": (8, -8), "full": (I64_MIN, I64_MAX), "2^53 alone": (P53, P53),
                  "-2^53 alone": (-P53, -P53), "hi on a value": (-7, P53 + 1), "lo on a value": (-(P53 + 1), 6),
                  "hi = max": (I64_MAX - 1, I64_MAX), "lo = min": (I64_MIN, I64_MIN + 1),
                  "hi just below a value": (0, P53)}
    for name, (lo, hi) in i64_ranges.items():
        cases.append(("i64 " + name, "i64", [(c, lo, hi) for c in W["i64"]]))
    f64_ranges = {"(-inf, inf)": (-np.inf, np.inf), "[inf, inf]": (np.inf, np.inf), "[-inf, -inf]": (-np.inf, -np.inf),
                  "[-0.0, 0.0]": (-0.0, 0.0), "[0.0, -0.0]": (0.0, -0.0), "on the values": (F64_LO, F64_HI),
                  "one ulp inside": (np.nextafter(F64_LO, np.inf), np.nextafter(F64_HI, -np.inf)),
                  "one ulp outside": (np.nextafter(F64_LO, -np.inf), np.nextafter(F64_HI, np.inf)),
                  "lo > hi": (1.0, -1.0)}
    for name, (lo, hi) in f64_ranges.items():
        cases.append(("f64 " + name, "f64", [(c, lo, hi) for c in W["f64"]]))
    T = W["terms"]
    for absent in (True, False):
        tag = "absent" if absent else "present"
        for j in range(T.shape[0]):
            cases.append((f"terms {tag} term {j}", "terms", [([T[j, s]], absent, None) for s in range(n_segs)]))
        cases.append((f"terms {tag} no term", "terms", [([], absent, None)] * n_segs))
        cases.append((f"terms {tag} two terms", "terms", [([T[1, s], T[4, s]], absent, None) for s in range(n_segs)]))
        odd = [np.arange(s.n_docs) % 2 == 1 for s in W["segs"]]
        odd[2] = None
        cases.append((f"terms {tag} and_masks", "terms", [([T[2, s], T[4, s]], absent, odd[s]) for s in range(n_segs)]))
    return cases


def f_updates(W):
    """-> {segment: (bitmap, live_docs)}: new tombstones for the segments of 65 and 1000 docs (a word's last bit, a
    word's first bit, doc 0; what was dead stays dead)"""
    out = {}
    for s, extra in ((F_DOCS.index(65), [0, 31, 32, 64]), (F_DOCS.index(1000), [0, 63, 255, 256, 511, 998])):
        seg = W["segs"][s]
        bits = np.zeros(seg.n_docs, dtype=bool)
        if seg.deleted is not None:
            bits |= np.unpackbits(seg.deleted, bitorder="little")[:seg.n_docs].astype(bool)
        bits[extra] = True
        out[s] = (np.packbits(bits, bitorder="little"), float(seg.n_docs - int(bits.sum())))
    return out


# ---- B: many postings ----------------------------------------------------------------------------------
B_DOCS, B_LISTS = 70_000, 31
B_GRID = 256 * 32 * 256  # threads of the largest staging grid: beyond it the kernel's loop takes a second turn


def b_segment():
    """31 lists of every doc: more postings than the staging grid has threads"""
    d = np.arange(B_DOCS, dtype=np.uint32)
    docs = np.tile(d, B_LISTS)
    t = np.repeat(np.arange(B_LISTS, dtype=np.uint32), B_DOCS)
    tfs = 1 + (docs * np.uint32(7) + t * np.uint32(13)) % np.uint32(23)
    lens = (5 + (np.arange(B_DOCS) * 31) % 97).astype(F32)
    return Segment(n_docs=B_DOCS, term_offsets=np.arange(B_LISTS + 1, dtype=np.uint64) * np.uint64(B_DOCS), doc_ids=docs,
                   tfs=tfs.astype(np.uint32), field_doc_len=[lens], field_avgdl=np.array([lens.mean()], dtype=F32),
                   docs=float(B_DOCS), k1=0.9, b=0.4)


def b_tombstones():
    dead = np.zeros(B_DOCS, dtype=bool)
    dead[::9] = True
    dead[B_DOCS - 1] = True
    return np.packbits(dead, bitorder="little"), float(B_DOCS - int(dead.sum()))
