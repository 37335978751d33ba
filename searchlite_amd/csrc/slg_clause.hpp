// slg_clause.hpp — what the two clause-filter kernels share (bool_filter_kernel, slg_bool.hpp;
// phrase_filter_kernel, slg_phrase.hpp): the parameters of a filter launch, the slice prologue, the binary
// searches of a lane's doc in several posting lists side by side, the pass over a query's term groups and the
// in-place compaction of the slice's candidate region.  Device helpers only: each unit compiles its own kernel.
//
// Shape of both kernels: one wave per slice, one candidate per lane, 64 candidates per chunk.  The query's
// BoolQuery and the (query, segment) row of BoolTerms are wave-uniform and are read through the constant
// address space (scalar loads): they cost no vector load per candidate.  The row holds MUST terms first,
// MUST_NOT second, SHOULD last, and the wave leaves the row as soon as a ballot shows every lane decided.
#pragma once

#include "slg_wave.hpp"

namespace slg {

struct BoolFilterParams {
  const SegDev *segs;
  const RoundQuery *sq;        // [n_sq] sub-queries: query and segment of a slice
  const uint32_t *slice_sq;    // [n_slices] sub-query of the slice
  const BoolQuery *queries;    // [nq] (a phrase batch: masks and min_should over ALL groups)
  const BoolTerm *terms;       // (slg_desc.hpp: [term_begin * n_segs + seg * n_terms + i])
  uint2 *cand;                 // {ordered score, doc} (doc 0xFFFFFFFF: dropped by the scoring kernel)
  const uint64_t *slice_cbeg;  // [n_slices] first candidate slot of the slice: read, never written
  uint32_t *slice_ccnt;        // [n_slices] candidates of the slice: rewritten
  uint32_t *q_scored;          // [nq] the clause table's rejects are taken off
  uint32_t n_slices, n_segs;
};

constexpr int kClauseListsPerStep = 4;  // binary searches a lane runs side by side

typedef const __attribute__((address_space(1))) uint32_t *clause_gu32_t;

// The uniforms of one slice, and the slice's survivors so far.
// (slice_sq, the sub-queries and the clause tables were uploaded when the batch was prepared; slice_cbeg and
//  slice_ccnt were written by the scoring kernel, which has finished: none of them changes under this wave's
//  loads, and this wave's own store to slice_ccnt[s] comes after its only load of it)
struct ClauseSlice {
  uint32_t q, seg;
  uint32_t nt;                       // clause terms of the query: the row's length
  uint32_t must, must_not, should;   // BoolQuery's masks
  uint32_t min_should, n_must;
  uint32_t n_rej_terms;              // MUST and MUST_NOT terms: behind them only SHOULD terms are left
  const BoolTerm *row;               // the (query, segment) row
  clause_gu32_t docs;                // the segment's doc ids
  uint32_t ccnt;                     // candidates of the slice
  uint2 *reg;                        // its candidate region
  uint32_t kept, rejected;
};

// the slice's query and segment and the query's clause record (the caller decides whether the query has work) ...
__device__ __forceinline__ ClauseSlice clause_query(const BoolFilterParams &p, uint32_t s) {
  ClauseSlice sl;
  const RoundQuery rq = load_const(p.sq + load_const(p.slice_sq + s));
  sl.q = rfl(rq.q);
  sl.seg = rfl(rq.seg);
  const BoolQuery bq = load_const(p.queries + sl.q);
  sl.nt = rfl(bq.n_terms);
  sl.must = rfl(bq.must_mask);
  sl.must_not = rfl(bq.must_not_mask);
  sl.should = rfl(bq.should_mask);
  sl.min_should = rfl(bq.min_should);
  sl.n_must = rfl(bq.n_must);
  sl.n_rej_terms = rfl(bq.n_must) + rfl(bq.n_must_not);
  sl.row = p.terms + ((size_t)rfl(bq.term_begin) * p.n_segs + (size_t)sl.seg * sl.nt);
  sl.kept = sl.rejected = 0u;
  return sl;
}
// ... and, for a query that has, the segment's lists and the slice's candidate region
__device__ __forceinline__ void clause_region(const BoolFilterParams &p, uint32_t s, ClauseSlice &sl) {
  const SegDev sd = load_const(p.segs + sl.seg);
  sl.docs = (clause_gu32_t)sd.docs;
  sl.ccnt = rfl(load_const(p.slice_ccnt + s));
  sl.reg = p.cand + uniform64(load_const(p.slice_cbeg + s));
}

// the candidate of slot i of the region (behind its end: a dropped entry)
__device__ __forceinline__ uint2 clause_candidate(const ClauseSlice &sl, uint32_t i) {
  uint2 c = make_uint2(0u, 0xFFFFFFFFu);
  if (i < sl.ccnt) c = sl.reg[i];
  return c;
}

// The doc of every lane in `on` searched in G lists side by side: list g is docs[off[g] .. off[g] + cnt[g]),
// off and cnt wave-uniform.  ceil(log2 cnt) dependent 4-byte loads narrow a list to one posting, one more
// compares it; the probes of the G lists are issued back to back before the first compare (a single search is
// a chain of dependent loads and a kernel would be latency-bound on it).  -> at[g]: the rank of the last
// posting <= doc in list g (or 0); hit[g]: that posting is doc (false for every lane outside `on`, whose doc
// may be kDocEnd).  Every probe lies in [off, off + cnt): the padding behind a list and the null run are never
// probed, and a list with cnt 0 is not read at all.
template <int G>
__device__ __forceinline__ void clause_search(const uint64_t (&off)[G], const uint32_t (&cnt)[G], clause_gu32_t docs,
                                              uint32_t doc, bool on, uint32_t (&at)[G], bool (&hit)[G]) {
  uint32_t n[G];
  bool more = false;
#pragma unroll
  for (int g = 0; g < G; g++) {
    n[g] = cnt[g];
    at[g] = 0u;
    more = more || n[g] > 1u;
  }
  while (more) {
    uint32_t v[G], half[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
      half[g] = n[g] >> 1;
      v[g] = 0xFFFFFFFFu;
      if (n[g] > 1u && on) v[g] = docs[off[g] + at[g] + half[g]];
    }
    more = false;
#pragma unroll
    for (int g = 0; g < G; g++) {
      if (n[g] > 1u) {
        at[g] = v[g] <= doc ? at[g] + half[g] : at[g];
        n[g] -= half[g];
      }
      more = more || n[g] > 1u;
    }
  }
  uint32_t hit_doc[G];
#pragma unroll
  for (int g = 0; g < G; g++) {
    hit_doc[g] = kDocEnd;
    if (n[g] != 0u && on) hit_doc[g] = docs[off[g] + at[g]];
  }
#pragma unroll
  for (int g = 0; g < G; g++) hit[g] = on && hit_doc[g] == doc;
}

// The term groups of one candidate per lane: the row's terms in steps of kClauseListsPerStep, each step's lists
// searched side by side.  must_t: the MUST groups that are term groups; terms_decide (uniform): the query has
// nothing but term groups, so the terms alone may accept.  -> held: bit g, a term of group g holds the doc
// (complete for the lanes the terms have not rejected).
__device__ __forceinline__ uint32_t clause_term_pass(const ClauseSlice &sl, uint32_t must_t, bool terms_decide,
                                                     uint32_t doc, bool live) {
  constexpr int G = kClauseListsPerStep;
  uint32_t held = 0;
  bool open = live;  // not decided yet: this lane still probes
  for (uint32_t ti = 0; ti < sl.nt; ti += G) {
    uint64_t off[G];
    uint32_t n[G], grp[G], at[G];
    bool hit[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
      const BoolTerm t = load_const(sl.row + (ti + g < sl.nt ? ti + g : ti));
      off[g] = uniform64(t.off);
      n[g] = ti + g < sl.nt ? rfl(t.df) : 0u;  // (uniform: the lanes of a wave search the same lists)
      grp[g] = rfl(t.group);
    }
    clause_search<G>(off, n, sl.docs, doc, open, at, hit);
#pragma unroll
    for (int g = 0; g < G; g++)
      if (hit[g]) held |= 1u << grp[g];
    // decided by the terms: rejected for good (a MUST_NOT group holds the doc; every MUST term was searched and a
    // MUST group of terms does not), or — terms_decide — accepted for good (only SHOULD terms are left and
    // enough SHOULD groups hold it)
    const uint32_t done = ti + G;
    const bool lost = (held & sl.must_not) != 0u || (done >= sl.n_must && (held & must_t) != must_t);
    const bool won = terms_decide && done >= sl.n_rej_terms && (held & sl.must) == sl.must &&
                     (uint32_t)__popc(held & sl.should) >= sl.min_should;
    open = open && !lost && !won;
    if (__ballot(open) == 0ull) break;
  }
  return held;
}

// the verdict on a candidate whose groups are all decided
__device__ __forceinline__ bool clause_accepts(const ClauseSlice &sl, uint32_t held, bool live) {
  return live && (held & sl.must) == sl.must && (held & sl.must_not) == 0u &&
         (uint32_t)__popc(held & sl.should) >= sl.min_should;
}

// The survivors of one chunk go back into the slice's region, IN PLACE from its start.  kept <= the chunk's
// first slot, so a chunk's writes land at or before the chunk's own first slot plus the lane's rank among the
// survivors, i.e. at or before the slot the lane read: a wave working front to back never overwrites a
// candidate it has not read (every lane of the chunk holds its candidate in registers before the first store:
// the accept ballot below).
__device__ __forceinline__ void clause_keep(ClauseSlice &sl, uint2 c, bool live, bool accept) {
  const uint64_t m = __ballot(accept);
  const uint32_t at = sl.kept + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  if (accept) sl.reg[at] = c;
  sl.kept += (uint32_t)__popcll(m);
  sl.rejected += (uint32_t)__popcll(__ballot(live && !accept));  // (a dropped entry is nobody's reject)
}
// the slice's new count, and its rejects off the query's scored docs
__device__ __forceinline__ void clause_finish(const BoolFilterParams &p, uint32_t s, const ClauseSlice &sl, uint32_t lane) {
  if (lane == 0u) {
    p.slice_ccnt[s] = sl.kept;  // (slice_cbeg stays: it is written for every slice and non-decreasing, as before)
    if (sl.rejected) atomicSub(&p.q_scored[sl.q], sl.rejected);
  }
}

}  // namespace slg
