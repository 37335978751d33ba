"""The bookkeeping of the few-term scoring kernel, restated in plain numpy / Python (test infrastructure).

score_uniform4_kernel (searchlite_amd/csrc/slg_score_uni4.hpp) cuts its slice into rounds, lays every round's postings
over 64 lanes of 8, streams a round that needs more lanes in chunks cut at a common doc, marks every loaded posting in
a filter whose fields repeat every 8 192 (4 list bits) or 4 096 docs (8 list bits), and joins the postings that found
another list's bit in their field.  This module predicts all of that structure from the posting lists and the planner's
tables (RoundQuery, TermRef).  It computes no score and no top-k: those come from the oracle.

  staged()      the padded posting array of a segment, as slg_index.hip lays it out (kListPad, kNullRun)
  slice_cuts()  the prologue's cut points of one slice, through the kernel's three search paths
  plain_cuts()  the same boundaries as one np.searchsorted statement
  lanes()       counts, lanes, first lanes and header bytes of a round
  chunks()      the chunk loop of an over-full round (f32 where the kernel computes in f32)
  wave()        the postings a wave loads for a round or chunk, their filter fields, the queue they form
  trace()       all of it for every sub-query of a plan; counters() the two per-query counters

The kernel's rules live in the module constants and in the four small functions `overfull`, `period`, `chunk_end`
and `before`, so that a one-line change of any of them is caught by the self-checks of tests/test_fewterm_worlds.py."""
import numpy as np

F32 = np.float32
DOC_END = 0xFFFFFFFF
NS = 8                 # kUniSlots: postings per lane
LANES = 64
LIST_PAD = 64          # kListPad: sentinels behind every list
NULL_RUN = 576         # kNullRun: sentinels at null_idx
FILTER_WORDS = 1024
TWO_PHASE_MIN = 9      # SLG_U4_TWO_PHASE_MIN
JOIN_PAIRS = 64        # SLG_U4_JOIN_PAIRS: queues up to this many entries are joined all-pairs
MAX_RPS = 16           # kMaxRoundsPerSlice


def overfull(total_lanes):
    return total_lanes > LANES


def period(ml):
    """docs after which the filter's fields repeat: 1 024 words x 8 fields of 4 bits, or x 4 fields of 8 bits"""
    return FILTER_WORDS * (8 if ml <= 4 else 4)


def field_key(doc, ml):
    """(word, field) of a doc as one number"""
    return doc % period(ml)


def chunk_end(bound, rend):
    return rend if bound == DOC_END else min(bound + 1, rend)


def before(doc, target):
    """a list is cut at its first posting with doc >= the boundary's doc: the postings before the cut are those below it"""
    return doc < target


def cut_words(ml):
    return 64 if ml <= 4 else 128


def lists_of(seg, term_ids):
    offs = np.asarray(seg.term_offsets, dtype=np.int64)
    docs = np.asarray(seg.doc_ids, dtype=np.int64)
    return [docs[offs[t]:offs[t + 1]] for t in term_ids]


def staged(seg):
    """the device's doc array: list t at term_offsets[t] + kListPad * t, kListPad sentinels behind it, kNullRun at the end"""
    offs = np.asarray(seg.term_offsets, dtype=np.int64)
    docs = np.asarray(seg.doc_ids, dtype=np.int64)
    V = len(offs) - 1
    out = np.full(int(offs[-1]) + LIST_PAD * V + NULL_RUN, DOC_END, dtype=np.int64)
    for t in range(V):
        out[offs[t] + LIST_PAD * t:offs[t + 1] + LIST_PAD * t] = docs[offs[t]:offs[t + 1]]
    return out


# ---- cut points ------------------------------------------------------------------------------------------------
def _window(d, df, target, a, NP):
    """lower_bound_window (slg_score.hpp): -> position, or None if the answer lies outside the 16 NP postings from a"""
    below = 0
    for i in range(NP + 1):
        at = a + 16 * i
        idx = at - 1 if 0 <= at - 1 < df else df
        v = int(d[0 if at == 0 else idx])
        below += 1 if (at == 0 or before(v, target)) else 0
    if below < 1 or below > NP:
        return None
    base = a + 16 * (below - 1)
    return base + int(before(d[base:base + 16], target).sum())


def _bisect(d, lo, hi, target):
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if before(d[mid], target):
            lo = mid + 1
        else:
            hi = mid
    return lo


def _guess(d, df, target, n_docs):
    """lower_bound_guess -> (position, path)"""
    g = min(df * target // max(n_docs, 1), df)
    pos = _window(d, df, target, g - 64 if g > 64 else 0, 8)
    if pos is not None:
        return pos, "guess"
    lo, hi, w = 0, df, 512
    while w < df:
        a = g - w if g > w else 0
        e = g + w if g + w < df else df
        if (a == 0 or before(d[a - 1], target)) and (e == df or not before(d[e - 1], target)):
            lo, hi = a, (df if e == df else e - 1)
            break
        w <<= 3
    return _bisect(d, lo, hi, target), "guess-bisect"


def slice_cuts(st, n_docs, tt, sq, r0, n_r):
    """the prologue of one slice (rounds r0 .. r0 + n_r of sub-query sq, inline cuts)
    -> (b[n_r + 1, T], rend[n_r], paths {(i, t): name}); paths: first / last / longest / guess / guess-bisect /
    window / bisect"""
    T, lg, nr_sq = len(tt), int(sq["longest"]), int(sq["n_rounds"])
    off = [int(x) for x in tt["off"]]
    df = [int(x) for x in tt["df"]]
    l_df = df[lg]
    stride = (l_df + nr_sq - 1) // nr_sq
    assert (n_r + 1) * T <= 128 and n_r <= MAX_RPS
    tgt, last_b = [], []
    for i in range(n_r + 1):
        j = r0 + i
        pos = j * stride
        mid = j != 0 and j < nr_sq and pos < l_df
        tgt.append(int(st[off[lg] + pos]) if mid else 0)
        last_b.append(j >= nr_sq or pos >= l_df)
    rend = [DOC_END if last_b[i] else tgt[i] for i in range(1, n_r + 1)]
    row0 = tgt[0]
    b = np.zeros((n_r + 1, T), dtype=np.int64)
    paths = {}

    def cut_one(i, t, target, inner):
        j = r0 + i
        if j == 0:
            return 0, "first"
        if last_b[i]:
            return df[t], "last"
        if t == lg:
            return j * stride, "longest"
        d = st[off[t]:]
        if not inner:
            return _guess(d, df[t], target, n_docs)
        lo, hi = int(b[0, t]), int(b[n_r, t])
        d1 = min(rend[n_r - 1], n_docs)
        fr = F32(target - row0) / F32(d1 - row0) if d1 > row0 else F32(0)
        g = min(lo + int(F32(hi - lo) * fr), hi)
        pos = _window(d, df[t], target, g - 32 if g > lo + 32 else lo, 4)
        if pos is not None:
            return pos, "window"
        return _bisect(d, lo, hi, target), "bisect"

    two_phase = n_r >= TWO_PHASE_MIN
    order = [0, n_r] + list(range(1, n_r)) if two_phase else list(range(n_r + 1))
    for i in order:
        for t in range(T):
            b[i, t], paths[(i, t)] = cut_one(i, t, tgt[i], two_phase and 0 < i < n_r)
    return b, rend, paths


def plain_cuts(L, longest, n_rounds):
    """boundary j of every list as one np.searchsorted statement -> b[n_rounds + 1, T]"""
    df = np.array([len(x) for x in L], dtype=np.int64)
    stride = (int(df[longest]) + n_rounds - 1) // n_rounds
    b = np.zeros((n_rounds + 1, len(L)), dtype=np.int64)
    for j in range(1, n_rounds + 1):
        if j >= n_rounds or j * stride >= df[longest]:
            b[j] = df
        else:
            b[j] = [np.searchsorted(x, L[longest][j * stride], side="left") for x in L]
    return b


# ---- rounds, chunks, waves -------------------------------------------------------------------------------------
def lanes(c):
    """counts of a round -> its lane layout and header"""
    c = np.asarray(c, dtype=np.int64)
    m = (c + NS - 1) // NS
    first = np.cumsum(m) - m
    total = int(m.sum())
    return dict(c=c, m=m, first=first, total=total, used=min(total, LANES), overfull=overfull(total),
                hdr_lanes=min(total, 255), first_bytes=np.minimum(first, 127))


def chunks(st, off, lo, hi, rend):
    """the chunk loop of an over-full round: -> [dict(cur, rem, nne, need, share, mlanes, chunk, lastdoc, bound, end,
    consumed)]"""
    T = len(off)
    cur, out = np.asarray(lo, dtype=np.int64).copy(), []
    hi = np.asarray(hi, dtype=np.int64)
    while True:
        rem = hi - cur
        R = int(rem.sum())
        if R == 0:
            break
        nne = int((rem != 0).sum())
        need = int(((rem + NS - 1) // NS).sum())
        chunk, share, mlanes = rem.copy(), np.zeros(T, dtype=F32), np.zeros(T, dtype=np.int64)
        if need > LANES:
            share = F32(LANES - nne) * (rem.astype(F32) / F32(R))
            mlanes = np.where(rem == 0, 0, 1 + share.astype(np.uint32).astype(np.int64))
            chunk = np.minimum(rem, mlanes * NS)
        lastdoc = [int(st[off[t] + cur[t] + chunk[t] - 1]) if chunk[t] < rem[t] else DOC_END for t in range(T)]
        bound = min(lastdoc)
        end = chunk_end(bound, rend)
        m = (chunk + NS - 1) // NS
        assert int(m.sum()) <= LANES, "a chunk is sized for 64 lanes"
        consumed = np.array([int((st[off[t] + cur[t]:off[t] + cur[t] + NS * m[t]] < end).sum()) for t in range(T)],
                            dtype=np.int64)
        assert consumed.sum() >= 1, "every chunk consumes at least one posting"
        assert (consumed <= chunk).all(), "a list consumes a prefix of its chunk"
        out.append(dict(cur=cur.copy(), rem=rem, nne=nne, need=need, share=share, mlanes=mlanes, chunk=chunk,
                        lastdoc=lastdoc, bound=bound, end=end, consumed=consumed, R=R))
        cur = cur + consumed
    return out


def wave(st, off, lo, cnt, end, ml):
    """what one wave loads and queues for the per-list ranges [lo, lo + cnt) with doc < end
    -> dict(doc, lst, pos, mine (inside its range), x (other lists' bits in the posting's field), queued, n, seg_len,
            partner, alias, idle_lanes)"""
    T = len(off)
    cnt = np.asarray(cnt, dtype=np.int64)
    m = (cnt + NS - 1) // NS
    doc = np.concatenate([st[off[t] + lo[t]:off[t] + lo[t] + NS * m[t]] for t in range(T)] + [np.zeros(0, np.int64)])
    lst = np.concatenate([np.full(NS * m[t], t, dtype=np.int64) for t in range(T)] + [np.zeros(0, np.int64)])
    pos = np.concatenate([lo[t] + np.arange(NS * m[t], dtype=np.int64) for t in range(T)] + [np.zeros(0, np.int64)])
    mine = pos < (np.asarray(lo, dtype=np.int64) + cnt)[lst] if len(lst) else np.zeros(0, dtype=bool)
    key = field_key(doc, ml)
    bits = {}
    for kk, t in zip(key.tolist(), lst.tolist()):
        bits[kk] = bits.get(kk, 0) | (1 << t)
    x = np.array([bits[kk] ^ (1 << t) for kk, t in zip(key.tolist(), lst.tolist())], dtype=np.int64)
    if T == 1:
        x[:] = 0
    queued = (x != 0) & (doc < end)
    qdoc, qlst = doc[queued], lst[queued]       # (list, position) order = lane-major
    same = {}
    for d in qdoc.tolist():
        same[d] = same.get(d, 0) + 1
    partner = np.array([same[d] > 1 for d in qdoc.tolist()], dtype=bool)
    return dict(doc=doc, lst=lst, pos=pos, mine=mine, x=x, queued=queued, n=int(queued.sum()), qdoc=qdoc, qlst=qlst,
                seg_len=np.bincount(qlst, minlength=T)[:T], partner=partner, alias=~partner,
                idle_lanes=LANES - int(m.sum()), below=int((doc < end).sum()), end=end)


def trace(segs, sqs, terms, ml):
    """every slice, round and wave of a plan on the few-term kernel; ml = 4 or 8, the kernel instance of the batch
    -> [dict(i, T, b (sub-query wide), slices=[dict(r0, n_r, b, rend, paths, rounds=[dict(lanes, waves, chunks)])])]"""
    out, cache = [], {}
    for i, sq in enumerate(sqs):
        T = int(sq["n_terms"])
        tt = terms[int(sq["term_begin"]):int(sq["term_begin"]) + T]
        s = int(sq["seg"])
        if s not in cache:
            cache[s] = staged(segs[s])
        st = cache[s]
        off = [int(x) for x in tt["off"]]
        nr, rps = int(sq["n_rounds"]), int(sq["rounds_per_slice"])
        assert (rps + 1) * T <= (cut_words(ml) if T > 4 else 64)
        slices, whole = [], np.zeros((nr + 1, T), dtype=np.int64)
        for r0 in range(0, nr, rps):
            n_r = min(rps, nr - r0)
            b, rend, paths = slice_cuts(st, segs[s].n_docs, tt, sq, r0, n_r)
            if r0:
                assert (whole[r0] == b[0]).all(), "two slices cut their common boundary differently"
            whole[r0:r0 + n_r + 1] = b
            rounds = []
            for r in range(n_r):
                ln = lanes(b[r + 1] - b[r])
                if ln["overfull"]:
                    ch = chunks(st, off, b[r], b[r + 1], rend[r])
                    waves = [wave(st, off, c["cur"], c["chunk"], c["end"], ml) for c in ch]
                    got = sum(c["consumed"] for c in ch)
                    assert (got == ln["c"]).all(), "the chunks of a round consume exactly the round"
                else:
                    ch, waves = [], [wave(st, off, b[r], ln["c"], rend[r], ml)]
                    assert waves[0]["below"] == int(ln["c"].sum()), "a round's postings are those below its end doc"
                rounds.append(dict(lanes=ln, waves=waves, chunks=ch, end=rend[r]))
            slices.append(dict(r0=r0, n_r=n_r, b=b, rend=rend, paths=paths, rounds=rounds))
        assert (whole[-1] == [int(x) for x in tt["df"]]).all(), "the last boundary is the end of every list"
        out.append(dict(i=i, T=T, b=whole, slices=slices, q=int(sq["q"]), seg=s, terms=[int(x) for x in tt["term"]],
                        longest=int(sq["longest"]), n_rounds=nr))
    return out


def counters(segs, traced, nq):
    """-> (distinct docs, postings) per query: slg_stats.scored_docs and postings_advanced of an unclassified run"""
    docs, postings = np.zeros(nq, dtype=np.int64), np.zeros(nq, dtype=np.int64)
    for sub in traced:
        L = lists_of(segs[sub["seg"]], sub["terms"])
        docs[sub["q"]] += len(np.unique(np.concatenate(L)))
        postings[sub["q"]] += sum(len(x) for x in L)
    return docs, postings
