// slg_phrase.hpp — phrase queries (slg_batch_prepare_phrase): the rest of the reference's accept()
// (QueryEvaluator::phrase_matches, api/reader.rs:1584-1597; matches_phrase, query/phrase.rs:4-48) as the one
// kernel a phrase batch runs between its scoring kernel and its select.  The semantics in full:
// include/searchlite_gpu.h.
//
// A phrase batch is a bool batch with one more kind of group: it runs in candidates mode, and
// phrase_filter_kernel evaluates the whole clause table of a query — its term groups, then its phrase groups —
// and compacts the slice's candidate region in place.  Every consumer behind it reads (slice_cbeg, slice_ccnt)
// and none of them changes.
//
// The kernel is bool_filter_kernel (slg_bool.hpp) with the variant loop between the term-group pass and the
// store of the survivors: the prologue, the pass, the side-by-side searches and the compaction are the
// clause-filter core both kernels share (slg_clause.hpp).  Per phrase group not yet decided, per variant that
// survives in the slice's segment:
//   (a) the doc is binary-searched in the variant's n <= 8 lists, four searches side by side; a miss ends the
//       variant for the lane;
//   (b) lanes with n hits load the n position ranges: the hit's place in the UNPADDED posting order is the
//       list's ubase plus its rank in the list, and offs[place], offs[place + 1] bound its positions;
//   (c) the chain test.  The predicate is: positions p0 < p1 < ... < p(n-1), p_i from list i, with
//       p(n-1) - p0 <= slop + n - 1.  For a start p0 the greedy picks, in every following list, the smallest
//       position above the previous pick: no chain from p0 ends earlier, so the greedy's last pick decides p0.
//       The picks are monotone in p0, so each list's cursor only moves forward over the starts — the work is
//       O(sum of the position counts) per doc, where the reference's depth-first search is exponential — and
//       when a list has no position above the previous pick no later start has one either: the lane stops.
// The cursors are indexed by compile-time constants only (unrolled to the 8-term limit, predicated on n), so
// they live in registers: the kernel uses no scratch and no LDS (nothing is shared between lanes).
#pragma once

#include "slg_clause.hpp"

namespace slg {

struct PhraseFilterParams {
  BoolFilterParams b;          // the slices, the candidates and the term groups' tables (queries: masks and
                               // min_should over ALL groups)
  const PosSegDev *pos_segs;   // [n_segs] of the batch's index state
  const PhraseQuery *pqueries; // [nq]
  const PhraseVar *vars;       // (slg_desc.hpp)
  const PhraseTerm *pterms;    // (slg_desc.hpp: [term_begin * n_segs + seg * n_terms + i])
};

constexpr int kPhraseThreads = 256;  // four waves = four slices per workgroup

// Terms BASE .. BASE + 3 of a variant (row = its first term, n its terms, uniform): the doc of every lane in
// `on` is searched in the four lists side by side, and for a hit the posting's position range goes to cur[] /
// end[].  -> the lane is still in: every list of this step that the variant has holds the doc with >= 1 position
template <int BASE>
__device__ __forceinline__ bool phrase_locate(const PhraseTerm *row, uint32_t n, clause_gu32_t docs, clause_gu32_t offs,
                                              uint32_t doc, bool on, uint32_t (&cur)[8], uint32_t (&end)[8]) {
  constexpr int G = kClauseListsPerStep;
  uint64_t off[G], ubase[G];
  uint32_t cnt[G], at[G];
  bool hit[G];
#pragma unroll
  for (int g = 0; g < G; g++) {
    const bool has = (uint32_t)(BASE + g) < n;
    const PhraseTerm t = load_const(row + (has ? BASE + g : 0));
    off[g] = uniform64(t.off);
    ubase[g] = uniform64(t.ubase);
    cnt[g] = has ? rfl(t.df) : 0u;  // (uniform: the lanes of a wave search the same lists)
  }
  clause_search<G>(off, cnt, docs, doc, on, at, hit);
  bool in = on;
#pragma unroll
  for (int g = 0; g < G; g++)
    if ((uint32_t)(BASE + g) < n) in = in && hit[g];
  // (b) the position ranges of the hits (a lane that missed a list loads nothing)
#pragma unroll
  for (int g = 0; g < G; g++) {
    cur[BASE + g] = 0u;
    end[BASE + g] = 0u;
    if ((uint32_t)(BASE + g) < n && in) {
      const uint64_t place = ubase[g] + at[g];
      cur[BASE + g] = offs[place];
      end[BASE + g] = offs[place + 1];
    }
  }
#pragma unroll
  for (int g = 0; g < G; g++)
    if ((uint32_t)(BASE + g) < n) in = in && cur[BASE + g] < end[BASE + g];  // an empty position list fails the variant
  return in;
}

// (c) the chain test of one lane: cur / end bound the n >= 2 position ranges, every one non-empty
__device__ __forceinline__ bool phrase_chain(clause_gu32_t pos, uint32_t n, uint32_t span, uint32_t (&cur)[8],
                                             const uint32_t (&end)[8]) {
  bool match = false, dead = false;
  while (!match && !dead && cur[0] < end[0]) {
    const uint32_t p0 = pos[cur[0]];
    uint32_t prev = p0;
#pragma unroll
    for (int i = 1; i < 8; i++) {
      if ((uint32_t)i < n && !dead) {
        uint32_t c = cur[i], v = 0u;
        bool got = false;
        while (c < end[i]) {  // the smallest position of list i above the previous pick
          v = pos[c];
          if (v > prev) {
            got = true;
            break;
          }
          c++;
        }
        cur[i] = c;  // (everything before c is <= this pick's predecessor, and the predecessors only grow)
        dead = !got;
        prev = got ? v : prev;
      }
    }
    match = !dead && prev - p0 <= span;
    cur[0]++;
  }
  return match;
}

static __global__ void __launch_bounds__(kPhraseThreads) phrase_filter_kernel(PhraseFilterParams p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = rfl(blockIdx.x * (kPhraseThreads / 64) + (threadIdx.x >> 6));
  if (s >= p.b.n_slices) return;
  // (the phrase tables were uploaded when the batch was prepared, the positions when the batch's index state
  //  was built: as the tables of ClauseSlice, none of them changes under this wave's loads)
  ClauseSlice sl = clause_query(p.b, s);
  if ((sl.must | sl.must_not | sl.should) == 0u) return;  // a query without a group is left as it is
  const PhraseQuery pq = load_const(p.pqueries + sl.q);
  const uint32_t nv = rfl(pq.n_vars);
  const uint32_t n_tg = rfl(pq.n_term_groups);
  const uint32_t must_t = sl.must & (n_tg >= 32u ? 0xFFFFFFFFu : (1u << n_tg) - 1u);  // the MUST groups of terms
  const PhraseVar *const vars = p.vars + rfl(pq.var_begin);
  const uint32_t npt = rfl(pq.n_terms);
  const PhraseTerm *const prow = p.pterms + ((size_t)rfl(pq.term_begin) * p.b.n_segs + (size_t)sl.seg * npt);
  clause_region(p.b, s, sl);
  const PosSegDev ps = load_const(p.pos_segs + sl.seg);
  const clause_gu32_t poffs = (clause_gu32_t)ps.offs, ppos = (clause_gu32_t)ps.pos;

  for (uint32_t base = 0; base < sl.ccnt; base += 64u) {
    const uint2 c = clause_candidate(sl, base + lane);
    const uint32_t doc = c.y;
    const bool live = doc != 0xFFFFFFFFu;  // (a dropped entry stays dropped)
    // ---- the term groups: a query without a variant is decided by them alone ----
    uint32_t held = clause_term_pass(sl, must_t, nv == 0u, doc, live);
    // ---- the phrase groups: a lane the terms rejected needs none of them ----
    bool open = live && (held & sl.must_not) == 0u && (held & must_t) == must_t;
    for (uint32_t vi = 0; vi < nv; vi++) {
      if (__ballot(open) == 0ull) break;
      const PhraseVar pv = load_const(vars + vi);
      const uint32_t n = rfl(pv.n_last) & 0xFFu, bit = 1u << rfl(pv.group);
      const PhraseTerm *const vrow = prow + rfl(pv.t_begin);
      const bool survives = rfl(load_const(&vrow->df)) != 0u;  // (uniform: dropped variants hold nothing)
      const bool need = open && (held & bit) == 0u;  // a group an earlier variant holds is decided
      if (survives && __ballot(need) != 0ull) {
        uint32_t cur[8], end[8];
        bool in = phrase_locate<0>(vrow, n, sl.docs, poffs, doc, need, cur, end);
        if (n > 4u) {
          in = phrase_locate<4>(vrow, n, sl.docs, poffs, doc, in, cur, end);
        } else {
#pragma unroll
          for (int g = 4; g < 8; g++) cur[g] = end[g] = 0u;
        }
        bool match = in;
        if (n > 1u && in) match = phrase_chain(ppos, n, rfl(pv.slop) + n - 1u, cur, end);
        if (match) held |= bit;
      }
      if ((rfl(pv.n_last) >> 8) != 0u) {  // the group is complete: a MUST that failed or a MUST_NOT that holds decides
        if ((sl.must & bit) != 0u) open = open && (held & bit) != 0u;
        if ((sl.must_not & bit) != 0u) open = open && (held & bit) == 0u;
      }
    }
    clause_keep(sl, c, live, clause_accepts(sl, held, live));
  }
  clause_finish(p.b, s, sl, lane);
}

}  // namespace slg
