// slg_phrase.hpp — phrase queries (slg_batch_prepare_phrase): the rest of the reference's accept()
// (QueryEvaluator::phrase_matches, api/reader.rs:1584-1597; matches_phrase, query/phrase.rs:4-48) as the one
// kernel a phrase batch runs between its scoring kernel and its select.  The semantics in full:
// include/searchlite_gpu.h.
//
// A phrase batch is a bool batch with one more kind of group: it runs in candidates mode, and
// phrase_filter_kernel evaluates the whole clause table of a query — its term groups exactly as
// bool_filter_kernel does (slg_bool.hpp; that part is repeated here, not shared, so that the bool kernel's code
// and registers stay what they were), then its phrase groups — and compacts the slice's candidate region in
// place.  Every consumer behind it reads (slice_cbeg, slice_ccnt) and none of them changes.
//
// Shape: one wave per slice, one candidate per lane, 64 candidates per chunk; the tables are wave-uniform and
// read through the constant address space.  Per phrase group not yet decided, per variant that survives in the
// slice's segment:
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

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_wave.hpp"

namespace slg {

struct PhraseFilterParams {
  const SegDev *segs;
  const PosSegDev *pos_segs;   // [n_segs] of the batch's index state
  const RoundQuery *sq;        // [n_sq] sub-queries: query and segment of a slice
  const uint32_t *slice_sq;    // [n_slices] sub-query of the slice
  const BoolQuery *queries;    // [nq] masks and min_should over ALL groups; the term groups' rows
  const BoolTerm *terms;       // (slg_desc.hpp: [term_begin * n_segs + seg * n_terms + i])
  const PhraseQuery *pqueries; // [nq]
  const PhraseVar *vars;       // (slg_desc.hpp)
  const PhraseTerm *pterms;    // (slg_desc.hpp: [term_begin * n_segs + seg * n_terms + i])
  uint2 *cand;                 // {ordered score, doc} (doc 0xFFFFFFFF: dropped by the scoring kernel)
  const uint64_t *slice_cbeg;  // [n_slices] first candidate slot of the slice: read, never written
  uint32_t *slice_ccnt;        // [n_slices] candidates of the slice: rewritten
  uint32_t *q_scored;          // [nq] the clause table's rejects are taken off
  uint32_t n_slices, n_segs;
};

constexpr int kPhraseThreads = 256;     // four waves = four slices per workgroup
constexpr int kPhraseListsPerStep = 4;  // binary searches a lane runs side by side

typedef const __attribute__((address_space(1))) uint32_t *phrase_gu32_t;

// a record that is written before the kernel starts and never during it, through the constant address space
template <typename T>
__device__ __forceinline__ T phrase_load_const(const T *src) {
  static_assert(sizeof(T) % 4 == 0, "whole words");
  typedef const __attribute__((address_space(4))) uint32_t *c_u32_t;
  const c_u32_t w = (c_u32_t)(uintptr_t)src;
  T out;
  uint32_t *dst = reinterpret_cast<uint32_t *>(&out);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 4; i++) dst[i] = w[i];
  return out;
}

__device__ __forceinline__ uint64_t phrase_uniform64(uint64_t v) {
  return ((uint64_t)rfl((uint32_t)(v >> 32)) << 32) | rfl((uint32_t)v);
}

// Terms BASE .. BASE + 3 of a variant (row = its first term, n its terms, uniform): the doc of every lane in
// `on` is searched in the four lists side by side, and for a hit the posting's position range goes to cur[] /
// end[].  -> the lane is still in: every list of this step that the variant has holds the doc with >= 1 position
template <int BASE>
__device__ __forceinline__ bool phrase_locate(const PhraseTerm *row, uint32_t n, phrase_gu32_t docs, phrase_gu32_t offs,
                                              uint32_t doc, bool on, uint32_t (&cur)[8], uint32_t (&end)[8]) {
  constexpr int G = kPhraseListsPerStep;
  uint64_t off[G], ubase[G];
  uint32_t cnt[G], at[G];
#pragma unroll
  for (int g = 0; g < G; g++) {
    const bool has = (uint32_t)(BASE + g) < n;
    const PhraseTerm t = phrase_load_const(row + (has ? BASE + g : 0));
    off[g] = phrase_uniform64(t.off);
    ubase[g] = phrase_uniform64(t.ubase);
    cnt[g] = has ? rfl(t.df) : 0u;  // (uniform: the lanes of a wave search the same lists)
    at[g] = 0u;
  }
  // the last posting <= doc of each list (or posting 0): every probe lies in [off, off + df)
  bool more = false;
#pragma unroll
  for (int g = 0; g < G; g++) more = more || cnt[g] > 1u;
  while (more) {
    uint32_t v[G], half[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
      half[g] = cnt[g] >> 1;
      v[g] = 0xFFFFFFFFu;
      if (cnt[g] > 1u && on) v[g] = docs[off[g] + at[g] + half[g]];
    }
    more = false;
#pragma unroll
    for (int g = 0; g < G; g++) {
      if (cnt[g] > 1u) {
        at[g] = v[g] <= doc ? at[g] + half[g] : at[g];
        cnt[g] -= half[g];
      }
      more = more || cnt[g] > 1u;
    }
  }
  uint32_t hit_doc[G];
#pragma unroll
  for (int g = 0; g < G; g++) {
    hit_doc[g] = kDocEnd;
    if (cnt[g] != 0u && on) hit_doc[g] = docs[off[g] + at[g]];
  }
  bool in = on;
#pragma unroll
  for (int g = 0; g < G; g++)
    if ((uint32_t)(BASE + g) < n) in = in && hit_doc[g] == doc;
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
__device__ __forceinline__ bool phrase_chain(phrase_gu32_t pos, uint32_t n, uint32_t span, uint32_t (&cur)[8],
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
  constexpr int G = kPhraseListsPerStep;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = rfl(blockIdx.x * (kPhraseThreads / 64) + (threadIdx.x >> 6));
  if (s >= p.n_slices) return;
  // (slice_sq, the sub-queries and the tables were uploaded when the batch was prepared, the positions when
  //  the batch's index state was built; slice_cbeg and slice_ccnt were written by the scoring kernel, which has
  //  finished: none of them changes under this wave's loads, and this wave's own store to slice_ccnt[s] comes
  //  after its only load of it)
  const RoundQuery rq = phrase_load_const(p.sq + phrase_load_const(p.slice_sq + s));
  const uint32_t q = rfl(rq.q), seg = rfl(rq.seg);
  const BoolQuery bq = phrase_load_const(p.queries + q);
  const uint32_t must = rfl(bq.must_mask), must_not = rfl(bq.must_not_mask), should = rfl(bq.should_mask);
  if ((must | must_not | should) == 0u) return;  // a query without a group is left as it is
  const PhraseQuery pq = phrase_load_const(p.pqueries + q);
  const uint32_t nt = rfl(bq.n_terms), nv = rfl(pq.n_vars);
  const uint32_t min_should = rfl(bq.min_should);
  const uint32_t n_rej_terms = rfl(bq.n_must) + rfl(bq.n_must_not);  // behind them only SHOULD terms are left
  const uint32_t n_must = rfl(bq.n_must);
  const uint32_t n_tg = rfl(pq.n_term_groups);
  const uint32_t must_t = must & (n_tg >= 32u ? 0xFFFFFFFFu : (1u << n_tg) - 1u);  // the MUST groups of terms
  const BoolTerm *const row = p.terms + ((size_t)rfl(bq.term_begin) * p.n_segs + (size_t)seg * nt);
  const PhraseVar *const vars = p.vars + rfl(pq.var_begin);
  const uint32_t npt = rfl(pq.n_terms);
  const PhraseTerm *const prow = p.pterms + ((size_t)rfl(pq.term_begin) * p.n_segs + (size_t)seg * npt);
  const SegDev sd = phrase_load_const(p.segs + seg);
  const PosSegDev ps = phrase_load_const(p.pos_segs + seg);
  const phrase_gu32_t docs = (phrase_gu32_t)sd.docs;
  const phrase_gu32_t poffs = (phrase_gu32_t)ps.offs, ppos = (phrase_gu32_t)ps.pos;
  const uint32_t ccnt = rfl(phrase_load_const(p.slice_ccnt + s));
  uint2 *const reg = p.cand + phrase_uniform64(phrase_load_const(p.slice_cbeg + s));

  uint32_t kept = 0, rejected = 0;
  for (uint32_t base = 0; base < ccnt; base += 64u) {
    const uint32_t i = base + lane;
    uint2 c = make_uint2(0u, 0xFFFFFFFFu);
    if (i < ccnt) c = reg[i];
    const uint32_t doc = c.y;
    const bool live = doc != 0xFFFFFFFFu;  // (a dropped entry stays dropped and is nobody's reject)
    uint32_t held = 0;
    bool open = live;  // not decided yet: this lane still probes
    // ---- the term groups: bool_filter_kernel's search, against the term groups' part of the masks ----
    for (uint32_t ti = 0; ti < nt; ti += G) {
      uint64_t off[G];
      uint32_t n[G], grp[G], pos[G];
#pragma unroll
      for (int g = 0; g < G; g++) {
        const BoolTerm t = phrase_load_const(row + (ti + g < nt ? ti + g : ti));
        off[g] = phrase_uniform64(t.off);
        n[g] = ti + g < nt ? rfl(t.df) : 0u;
        grp[g] = rfl(t.group);
        pos[g] = 0u;
      }
      bool more = false;
#pragma unroll
      for (int g = 0; g < G; g++) more = more || n[g] > 1u;
      while (more) {
        uint32_t v[G], half[G];
#pragma unroll
        for (int g = 0; g < G; g++) {
          half[g] = n[g] >> 1;
          v[g] = 0xFFFFFFFFu;
          if (n[g] > 1u && open) v[g] = docs[off[g] + pos[g] + half[g]];
        }
        more = false;
#pragma unroll
        for (int g = 0; g < G; g++) {
          if (n[g] > 1u) {
            pos[g] = v[g] <= doc ? pos[g] + half[g] : pos[g];
            n[g] -= half[g];
          }
          more = more || n[g] > 1u;
        }
      }
      uint32_t hit_doc[G];
#pragma unroll
      for (int g = 0; g < G; g++) {
        hit_doc[g] = kDocEnd;
        if (n[g] != 0u && open) hit_doc[g] = docs[off[g] + pos[g]];
      }
#pragma unroll
      for (int g = 0; g < G; g++)
        if (open && hit_doc[g] == doc) held |= 1u << grp[g];
      // decided by the terms alone: rejected for good (a MUST_NOT group holds the doc; every MUST term was
      // searched and a MUST group of terms does not), or — a query without a variant — accepted for good
      const uint32_t done = ti + G;
      const bool must_ok = (held & must_t) == must_t;
      const bool lost = (held & must_not) != 0u || (done >= n_must && !must_ok);
      const bool won = nv == 0u && done >= n_rej_terms && (held & must) == must &&
                       (uint32_t)__popc(held & should) >= min_should;
      open = open && !lost && !won;
      if (__ballot(open) == 0ull) break;
    }
    // ---- the phrase groups: a lane the terms rejected needs none of them ----
    open = live && (held & must_not) == 0u && (held & must_t) == must_t;
    for (uint32_t vi = 0; vi < nv; vi++) {
      if (__ballot(open) == 0ull) break;
      const PhraseVar pv = phrase_load_const(vars + vi);
      const uint32_t n = rfl(pv.n_last) & 0xFFu, bit = 1u << rfl(pv.group);
      const PhraseTerm *const vrow = prow + rfl(pv.t_begin);
      const bool survives = rfl(phrase_load_const(&vrow->df)) != 0u;  // (uniform: dropped variants hold nothing)
      const bool need = open && (held & bit) == 0u;  // a group an earlier variant holds is decided
      if (survives && __ballot(need) != 0ull) {
        uint32_t cur[8], end[8];
        bool in = phrase_locate<0>(vrow, n, docs, poffs, doc, need, cur, end);
        if (n > 4u) {
          in = phrase_locate<4>(vrow, n, docs, poffs, doc, in, cur, end);
        } else {
#pragma unroll
          for (int g = 4; g < 8; g++) cur[g] = end[g] = 0u;
        }
        bool match = in;
        if (n > 1u && in) match = phrase_chain(ppos, n, rfl(pv.slop) + n - 1u, cur, end);
        if (match) held |= bit;
      }
      if ((rfl(pv.n_last) >> 8) != 0u) {  // the group is complete: a MUST that failed or a MUST_NOT that holds decides
        if ((must & bit) != 0u) open = open && (held & bit) != 0u;
        if ((must_not & bit) != 0u) open = open && (held & bit) == 0u;
      }
    }
    const bool accept = live && (held & must) == must && (held & must_not) == 0u &&
                        (uint32_t)__popc(held & should) >= min_should;
    const uint64_t m = __ballot(accept);
    const uint32_t at = kept + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    // IN PLACE, as in bool_filter_kernel: kept <= base, so a chunk's writes land at or before the slots the
    // chunk read, and every lane of the chunk holds its candidate in registers before the first store (the
    // accept ballot above): a wave working front to back never overwrites a candidate it has not read.
    if (accept) reg[at] = c;
    kept += (uint32_t)__popcll(m);
    rejected += (uint32_t)__popcll(__ballot(live && !accept));
  }
  if (lane == 0u) {
    p.slice_ccnt[s] = kept;  // (slice_cbeg stays: it is written for every slice and non-decreasing, as before)
    if (rejected) atomicSub(&p.q_scored[q], rejected);
  }
}

}  // namespace slg
