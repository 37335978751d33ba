"""Plain references for what slg_stage.hpp stages once per segment version: the per-posting impacts, the
per-term champion table and the reject bitmaps of the bitmap, range and term filters (test infrastructure).

impacts() asks the oracle for every posting; impacts_np() restates the same path (ScoredTerm::doc_len
query/wand.rs:77-84, score_tf :279-285, bm25 query/bm25.rs:1-6) in numpy, one f32 operation at a time;
tests/test_stage_ref.py pins the two on each other bit for bit.  check_champions() states what the planner
needs of a champion table: row[0] is used as an upper bound and must be the exact maximum, every other entry
is used as a lower bound of an order statistic and may be low, never high."""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
CHAMP_SORTED = 64                    # entries 0..63: exact-rank lower bounds (slg_desc.hpp kChampSorted)
CHAMP_RANKS = (128, 256, 512, 1024)  # entries 64..67 bound these ranks
CHAMP_ROW = CHAMP_SORTED + len(CHAMP_RANKS)


def deleted_mask(seg) -> np.ndarray:
    if seg.deleted is None:
        return np.zeros(seg.n_docs, dtype=bool)
    return np.unpackbits(seg.deleted, bitorder="little")[:seg.n_docs].astype(bool)


def posting_terms(seg) -> np.ndarray:
    """term of every posting"""
    return np.repeat(np.arange(seg.n_terms), np.diff(seg.term_offsets.astype(np.int64)))


def doc_len(seg, field: int, doc: int) -> float:
    """ScoredTerm::doc_len (query/wand.rs:77-84): the stored length when there is one above 0, else max(avgdl, 1)"""
    lens = seg.field_doc_len[field]
    if lens is not None and doc < len(lens) and lens[doc] > 0.0:
        return float(lens[doc])
    return float(max(F32(seg.field_avgdl[field]), F32(1.0)))


def impacts(oracle, seg) -> np.ndarray:
    """f32[P]: the impact of every posting, one oracle.score_tf call each at weight 1; df = the list's length,
    docs = seg.docs"""
    out = np.zeros(seg.n_postings, dtype=F32)
    for t in range(seg.n_terms):
        a, b = int(seg.term_offsets[t]), int(seg.term_offsets[t + 1])
        f = 0 if seg.term_field is None else int(seg.term_field[t])
        avgdl = float(seg.field_avgdl[f])
        for i in range(a, b):
            out[i] = oracle.score_tf(float(F32(seg.tfs[i])), float(b - a), doc_len(seg, f, int(seg.doc_ids[i])), avgdl,
                                     seg.docs, seg.k1, seg.b, 1.0)
    return out


def idf_np(docs, df) -> F32:
    """bm25.rs:2: ((docs - df + 0.5) / (df + 0.5)).ln().max(0.0) + 1.0; f32::max ignores the NaN of a negative
    argument.  ln: the correctly rounded f32 logarithm (the double logarithm rounded once more)."""
    docs, df, half = F32(docs), F32(df), F32(0.5)
    with np.errstate(all="ignore"):
        arg = F32(F32(F32(docs - df) + half) / F32(df + half))
    if arg < 0 or math.isnan(arg):
        ln = F32(np.nan)
    elif arg == 0:
        ln = F32(-np.inf)
    else:
        ln = F32(math.log(float(arg))) if math.isfinite(arg) else F32(arg)
    return F32(np.fmax(ln, F32(0.0)) + F32(1.0))


def impacts_np(seg) -> np.ndarray:
    """impacts() restated in numpy: every line is one f32 operation over all postings"""
    term = posting_terms(seg)
    df = np.diff(seg.term_offsets.astype(np.int64))
    field = np.zeros(seg.n_postings, dtype=np.int64) if seg.term_field is None else seg.term_field[term].astype(np.int64)
    doc = seg.doc_ids.astype(np.int64)
    avgdl = seg.field_avgdl.astype(F32)[field]
    tf = seg.tfs.astype(F32)
    k1, b, one = F32(seg.k1), F32(seg.b), F32(1.0)
    idf = np.array([idf_np(seg.docs, d) for d in df], dtype=F32)[term]
    with np.errstate(all="ignore"):
        # doc_len(): the stored length above 0, else max(avgdl, 1)
        dl = np.fmax(avgdl, one)
        for f, lens in enumerate(seg.field_doc_len):
            if lens is None:
                continue
            at = np.nonzero((field == f) & (doc < len(lens)))[0]
            v = lens.astype(F32)[doc[at]]
            dl[at] = np.where(v > 0, v, dl[at])
        # score_tf
        norm_len = np.where(dl > 0, dl, np.fmax(avgdl, tf)).astype(F32)
        # bm25
        ratio = (norm_len / np.where(avgdl > 0, avgdl, one)).astype(F32)
        norm_dl = np.where(avgdl > 0, ratio, one).astype(F32)
        x = (b * norm_dl).astype(F32)
        x = (F32(one - b) + x).astype(F32)
        x = (k1 * x).astype(F32)
        denom = (tf + x).astype(F32)
        num = (tf * F32(k1 + one)).astype(F32)
        num = (idf * num).astype(F32)
        return (num / np.fmax(denom, F32(1e-6))).astype(F32)


# ---- champions -----------------------------------------------------------------------------------------
def lane_table(imps: np.ndarray) -> np.ndarray:
    """A table row that meets check_champions for a list with these live impacts in posting order (0 for a dead
    posting): posting i goes to lane i % 64; the sorted lane maxima, then the minimum over lanes of each lane's 2nd,
    4th, 8th and 16th largest.  What hand-made tables of the CPU test start from."""
    lanes = np.zeros((64, 16), dtype=F32)
    for l in range(64):
        top = np.sort(np.asarray(imps[l::64], dtype=F32))[::-1][:16]
        lanes[l, :len(top)] = top
    row = np.zeros(CHAMP_ROW, dtype=F32)
    row[:64] = np.sort(lanes[:, 0])[::-1]
    for j in range(4):
        row[64 + j] = lanes[:, 2 ** (j + 1) - 1].min()
    return row


def check_champions(table, seg, imps, what=""):
    """Asserts, per term over its live postings, what the planner relies on (module docstring).  imps: the
    impacts of seg's postings (impacts())."""
    table = np.asarray(table, dtype=F32)
    assert table.shape == (seg.n_terms, CHAMP_ROW), f"{what}: shape {table.shape}"
    dead = deleted_mask(seg)
    bits = lambda x: np.asarray(x, dtype=F32).view(np.uint32)
    for t in range(seg.n_terms):
        a, b = int(seg.term_offsets[t]), int(seg.term_offsets[t + 1])
        row, tag = table[t], f"{what} term {t} (df {b - a})"
        live = np.where(dead[seg.doc_ids[a:b]], F32(0.0), imps[a:b]).astype(F32)  # in posting order, dead = 0
        assert not np.isnan(row).any() and (row >= 0).all(), tag
        desc = np.sort(live[~dead[seg.doc_ids[a:b]]])[::-1]
        stat = lambda r: desc[r - 1] if r <= len(desc) else F32(0.0)  # the r-th largest live impact, 0 past the list
        # the upper bound: exact
        assert bits(row[0]) == bits(stat(1)), f"{tag}: row[0] {row[0]!r} is not the maximum {stat(1)!r}"
        # the lower bounds: never above their order statistic
        assert (np.diff(row[:64]) <= 0).all(), f"{tag}: entries 0..63 increase"
        for r in range(64):
            assert row[r] <= stat(r + 1), f"{tag}: row[{r}] {row[r]!r} > the {r + 1}-th largest {stat(r + 1)!r}"
        for j, rank in enumerate(CHAMP_RANKS):
            assert row[64 + j] <= stat(rank), f"{tag}: row[{64 + j}] {row[64 + j]!r} > the {rank}-th largest {stat(rank)!r}"
        # where a positive bound is due: posting i sits in lane i % 64; entry r needs r + 1 lanes with a live positive
        # posting, entry 64 + j needs 2^(j+1) of them in every lane.  Without tombstones and with positive impacts
        # only: row[r] > 0 exactly for r < min(df, 64), row[64 + j] > 0 exactly when df >= 128 * 2^j
        per_lane = np.array([int((live[l::64] > 0).sum()) for l in range(64)])
        n_lanes = int((per_lane > 0).sum())
        assert np.array_equal(row[:64] > 0, np.arange(64) < n_lanes), f"{tag}: positive entries {int((row[:64] > 0).sum())}, lanes {n_lanes}"
        for j in range(4):
            assert (row[64 + j] > 0) == (per_lane.min() >= 2 ** (j + 1)), f"{tag}: row[{64 + j}] = {row[64 + j]!r}, fewest per lane {per_lane.min()}"
        # all live impacts equal: every positive entry is that value
        if len(desc) and bits(desc[0]) == bits(desc[-1]):
            pos = row[row > 0]
            assert (bits(pos) == bits(desc[0])).all(), f"{tag}: entries differ from the list's one impact {desc[0]!r}"


# ---- the bitmap, range and term filters ----------------------------------------------------------------
def filter_pass(kind: str, args, seg) -> np.ndarray:
    """bool[n_docs]: the docs that are alive and pass.  kind "bitmap": args = mask or None; "i64" / "f64": (column,
    lo, hi), lo <= v <= hi in the column's own type (NaN never passes); "terms": (term ids of this segment with
    NO_TERM for absent ones, pass_if_absent, and_mask or None): the docs that hold none / at least one of the terms."""
    n = seg.n_docs
    if kind == "bitmap":
        ok = np.ones(n, dtype=bool) if args is None else np.asarray(args, dtype=bool).copy()
    elif kind == "i64":
        col, lo, hi = args
        col = np.asarray(col)
        assert col.dtype == np.int64
        ok = (col >= np.int64(lo)) & (col <= np.int64(hi))
    elif kind == "f64":
        col, lo, hi = args
        col = np.asarray(col)
        assert col.dtype == np.float64
        with np.errstate(invalid="ignore"):
            ok = (col >= np.float64(lo)) & (col <= np.float64(hi))
    elif kind == "terms":
        ids, pass_if_absent, and_mask = args
        held = np.zeros(n, dtype=bool)
        for t in ids:
            if int(t) != 0xFFFFFFFF:
                held[seg.postings(int(t))[0]] = True
        ok = ~held if pass_if_absent else held
        if and_mask is not None:
            ok = ok & np.asarray(and_mask, dtype=bool)
    else:
        raise ValueError(kind)
    return ok & ~deleted_mask(seg)
