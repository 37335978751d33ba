"""The control flow of the many-term scoring kernel, restated in plain numpy / Python (test infrastructure).

score_multi_kernel (searchlite_amd/csrc/slg_score_multi.hpp) works through planned rounds; a round that does not fit
the kernel's 512 accumulators, the 63 slot descriptors of a wave or the 16 384-doc bitmap window is cut at a common
doc id and finished in further chunks.  This module predicts, from the posting lists and the plan alone, every chunk
the kernel forms and the two counters it exports: the docs it scored (slg_stats.scored_docs) and the postings of
block-skipped slots it never loaded (PreparedBatch.skip_counts()).  It scores nothing: scores come from the oracle.

  rounds()    partition_rounds_kernel (slg_kernels.hpp): the cut points of every list at every round boundary
  chunks()    the chunk loop of score_multi_kernel: one record per chunk, per round
  counters()  scored docs and skipped postings per query, summed over its sub-queries' chunks

The float steps of the proportional cut are f32, as in the kernel."""
import numpy as np

F32 = np.float32
DOC_END = 0xFFFFFFFF
CAP = 512          # kMultiCap: accumulators (= distinct docs) of a chunk
FILL = 448         # kMultiFill: postings taken when a round has to be cut
SPAN = 16384       # kSpan: docs of the bitmap window
SLOT = 64          # postings of a slot
MAX_SLOTS = 60     # a chunk with more slots over all lists is cut (S_all > 60)
LANES = 63         # slot descriptors that the cut leaves room for


def lists_of(seg, term_ids):
    """the posting lists (doc ids, ascending) of the terms"""
    offs = np.asarray(seg.term_offsets, dtype=np.int64)
    docs = np.asarray(seg.doc_ids, dtype=np.int64)
    return [docs[offs[t]:offs[t + 1]] for t in term_ids]


def rounds(seg, term_ids, n_rounds, longest):
    """-> (bounds[n_rounds + 1, T], rdoc[n_rounds + 1]): list t's postings [bounds[j, t], bounds[j + 1, t]) and the
    docs [rdoc[j], rdoc[j + 1]) belong to round j"""
    L = lists_of(seg, term_ids)
    T = len(L)
    df = np.array([len(x) for x in L], dtype=np.int64)
    df_l = int(df[longest])
    stride = (df_l + n_rounds - 1) // n_rounds
    bounds = np.zeros((n_rounds + 1, T), dtype=np.int64)
    rdoc = np.zeros(n_rounds + 1, dtype=np.int64)
    for j in range(n_rounds + 1):
        pos = j * stride
        if j == 0:
            rdoc[j] = min(int(x[0]) for x in L)
        elif j >= n_rounds or pos >= df_l:
            bounds[j] = df
            rdoc[j] = max(int(x[-1]) for x in L) + 1
        else:
            target = int(L[longest][pos])
            for t in range(T):
                bounds[j, t] = pos if t == longest else int(np.searchsorted(L[t], target, side="left"))
            rdoc[j] = target
    return bounds, rdoc


def chunks(seg, term_ids, weights, bounds, rdoc, ess_mask, skip_mask, block_skip):
    """-> per round the list of its chunk records (dicts).  `weights` is not read: the model scores nothing.
    block_skip: the batch is MaxScore-classified and the index allows block skipping (RoundScoreParams::block_skip).
    A round (or the rest of one) without an essential posting is one record {"no_essential": True, R, n_skipped}."""
    L = lists_of(seg, term_ids)
    T = len(L)
    ess = np.array([(int(ess_mask) >> t) & 1 for t in range(T)], dtype=bool)
    skp = np.array([(int(skip_mask) >> t) & 1 for t in range(T)], dtype=bool) if block_skip else np.zeros(T, dtype=bool)
    skipping = bool(skp.any())
    out = []
    for r in range(len(rdoc) - 1):
        recs = []
        cur, end = bounds[r].astype(np.int64).copy(), bounds[r + 1].astype(np.int64)
        dlo, rdhi = int(rdoc[r]), int(rdoc[r + 1])
        while True:
            rem = end - cur
            R = int(rem.sum())
            if R == 0:
                break
            R_ess = int(rem[ess].sum())
            if block_skip and R_ess == 0:
                recs.append(dict(no_essential=True, R=R, R_ess=0, n_skipped=R, ndocs=0, consumed=rem.copy()))
                break
            S_all = int(((rem + 63) // 64).sum())
            chunk, dhi = rem.copy(), rdhi
            by_acc, by_slots, share, share_acc = R_ess > CAP, S_all > MAX_SLOTS, F32(1.0), F32(1.0)
            if by_acc or by_slots:
                if by_acc:
                    share = share_acc = F32(FILL) / F32(R_ess)
                if by_slots:
                    share = min(share, F32((LANES - T) * 64) / F32(R))
                c = (rem.astype(F32) * F32(share)).astype(np.uint32).astype(np.int64)   # truncated
                c = np.maximum(c, 1)
                chunk = np.minimum(rem, c)
                last = [int(L[t][cur[t] + chunk[t] - 1]) for t in range(T) if chunk[t] < rem[t]]
                dhi = min(last) + 1 if last else rdhi
            wbase = dlo & ~31
            by_window = dhi - wbase > SPAN
            if by_window:
                dhi = wbase + SPAN
            cut = by_acc or by_slots or by_window
            part = [L[t][cur[t]:cur[t] + chunk[t]] for t in range(T)]
            live = [p[p < dhi] for p in part]
            S = int(((chunk + 63) // 64).sum())
            S_a = int(((chunk[ess] + 63) // 64).sum())
            nb_a, nb = (S_a + 7) // 8, (S + 7) // 8
            edocs = np.unique(np.concatenate([live[t] for t in range(T) if ess[t]] + [np.zeros(0, np.int64)]))
            ndocs = len(edocs)
            slots, G, n_skipped, kept, first8_same = [], 0, 0, S, True
            for t in range(T):
                for s in range(int((chunk[t] + 63) // 64)):
                    if skipping and skp[t]:
                        cnt = int(min(64, chunk[t] - 64 * s))
                        fd, ld = int(part[t][64 * s]), int(part[t][64 * s + cnt - 1])
                        past, whole = fd >= dhi, ld < dhi
                        hits = 0 if past else int(np.searchsorted(edocs, min(ld, dhi - 1), side="right") -
                                                  np.searchsorted(edocs, fd, side="left"))
                        skipped = past or (whole and hits == 0)
                        slots.append(dict(list=t, G=G, s=s, cnt=cnt, fd=fd, ld=ld, hits=hits, skipped=skipped,
                                          kind="past" if past else "whole" if whole else "straddling"))
                        if skipped:
                            kept -= 1
                            first8_same = first8_same and G >= 8
                            n_skipped += cnt if whole else 0
                    G += 1
            consumed = np.array([len(x) for x in live], dtype=np.int64) if cut else rem.copy()
            recs.append(dict(no_essential=False, R=R, R_ess=R_ess, S_all=S_all, by_acc=by_acc, by_slots=by_slots,
                             by_window=by_window, cut=cut, share=share, share_acc=share_acc, rem=rem.copy(), chunk=chunk,
                             dlo=dlo, wbase=wbase, dhi=dhi, rdhi=rdhi, S=S, S_a=S_a, nb_a=nb_a, nb=nb,
                             nb_after=(kept + 7) // 8 if kept < S else nb, kept=kept, slots=slots,
                             first8_same=first8_same, ndocs=ndocs, edocs=edocs, consumed=consumed, n_skipped=n_skipped,
                             live=[len(x) for x in live]))
            if not cut:
                break
            cur = cur + consumed
            first = [int(L[t][cur[t]]) for t in range(T) if cur[t] < end[t]]
            if not first:
                break
            assert min(first) >= dhi and consumed.sum() > 0, "the model's chunk loop must advance"
            dlo = min(first)
        out.append(recs)
    return out


def trace(segs, sqs, terms, block_skip):
    """the chunk records of every sub-query of a plan: sqs / terms are the planner's RoundQuery / TermRef arrays
    -> [(sub-query index, bounds, rdoc, chunks())]"""
    out = []
    for i, sq in enumerate(sqs):
        tt = terms[int(sq["term_begin"]):int(sq["term_begin"]) + int(sq["n_terms"])]
        seg = segs[int(sq["seg"])]
        ids = [int(x) for x in tt["term"]]
        bounds, rdoc = rounds(seg, ids, int(sq["n_rounds"]), int(sq["longest"]))
        out.append((i, bounds, rdoc, chunks(seg, ids, tt["weight"], bounds, rdoc, int(sq["ess_mask"]),
                                            int(sq["skip_mask"]), block_skip)))
    return out


def counters(sqs, traced, nq):
    """-> (scored_docs[nq], skipped_postings[nq]) from trace()'s records"""
    scored, skipped = np.zeros(nq, dtype=np.int64), np.zeros(nq, dtype=np.int64)
    for i, _, _, per_round in traced:
        q = int(sqs[i]["q"])
        for recs in per_round:
            for c in recs:
                scored[q] += c["ndocs"]
                skipped[q] += c["n_skipped"]
    return scored, skipped
