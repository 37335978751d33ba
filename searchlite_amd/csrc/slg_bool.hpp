// slg_bool.hpp — boolean queries (slg_batch_prepare_bool): the clause test of the reference's accept()
// (QueryEvaluator::matches_node, api/reader.rs:1485-1565; term_group_matches, :1571-1580) as one kernel
// between the scoring kernel and the select.  The semantics in full: include/searchlite_gpu.h.
//
// A bool batch runs in candidates mode: the scoring kernel leaves every doc of the scored lists, with its
// exact score, in the region (slice_cbeg[s], slice_ccnt[s]) of its slice.  bool_filter_kernel tests every
// candidate against the query's clause table, writes the survivors back to the front of the same region and
// stores the new slice_ccnt — the one format every consumer behind it reads (the selects, and whatever else
// reads regions), so none of them changes.
//
// Shape: one wave per slice, one candidate per lane, 64 candidates per chunk.  The query's BoolQuery and the
// (query, segment) row of BoolTerms are wave-uniform and are read through the constant address space (scalar
// loads): they cost no vector load per candidate.  For every clause term with df > 0 a lane runs a binary
// search of its doc over docs[off .. off + df) — ceil(log2 df) dependent 4-byte loads narrow the list to one
// posting, one more compares it; the padding behind a list and the null run are never probed.  The searches
// of kBoolTermsPerStep terms run side by side (their probes are issued back to back before the first
// compare): a single search is a chain of dependent loads and the kernel would be latency-bound on it.
// The row holds MUST terms first, MUST_NOT second, SHOULD last, and the wave leaves the row as soon as a
// ballot shows every lane decided.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_wave.hpp"

namespace slg {

struct BoolFilterParams {
  const SegDev *segs;
  const RoundQuery *sq;        // [n_sq] sub-queries: query and segment of a slice
  const uint32_t *slice_sq;    // [n_slices] sub-query of the slice
  const BoolQuery *queries;    // [nq]
  const BoolTerm *terms;       // (slg_desc.hpp: [term_begin * n_segs + seg * n_terms + i])
  uint2 *cand;                 // {ordered score, doc} (doc 0xFFFFFFFF: dropped by the scoring kernel)
  const uint64_t *slice_cbeg;  // [n_slices] first candidate slot of the slice: read, never written
  uint32_t *slice_ccnt;        // [n_slices] candidates of the slice: rewritten
  uint32_t *q_scored;          // [nq] the clause table's rejects are taken off
  uint32_t n_slices, n_segs;
};

constexpr int kBoolThreads = 256;       // four waves = four slices per workgroup
constexpr int kBoolTermsPerStep = 4;    // binary searches a lane runs side by side

// a record that is written before the kernel starts and never during it, through the constant address space
template <typename T>
__device__ __forceinline__ T bool_load_const(const T *src) {
  static_assert(sizeof(T) % 4 == 0, "whole words");
  typedef const __attribute__((address_space(4))) uint32_t *c_u32_t;
  const c_u32_t w = (c_u32_t)(uintptr_t)src;
  T out;
  uint32_t *dst = reinterpret_cast<uint32_t *>(&out);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 4; i++) dst[i] = w[i];
  return out;
}

static __global__ void __launch_bounds__(kBoolThreads) bool_filter_kernel(BoolFilterParams p) {
  constexpr int G = kBoolTermsPerStep;
  typedef const __attribute__((address_space(1))) uint32_t *gdoc_t;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = rfl(blockIdx.x * (kBoolThreads / 64) + (threadIdx.x >> 6));
  if (s >= p.n_slices) return;
  // (slice_sq, the sub-queries and the clause tables were uploaded when the batch was prepared; slice_cbeg and
  //  slice_ccnt were written by the scoring kernel, which has finished: none of them changes under this wave's
  //  loads, and this wave's own store to slice_ccnt[s] comes after its only load of it)
  const RoundQuery rq = bool_load_const(p.sq + bool_load_const(p.slice_sq + s));
  const uint32_t q = rfl(rq.q), seg = rfl(rq.seg);
  const BoolQuery bq = bool_load_const(p.queries + q);
  const uint32_t nt = rfl(bq.n_terms);
  if (nt == 0u) return;  // a query without a clause table is left as it is
  const uint32_t must = rfl(bq.must_mask), must_not = rfl(bq.must_not_mask), should = rfl(bq.should_mask);
  const uint32_t min_should = rfl(bq.min_should);
  const uint32_t n_rej_terms = rfl(bq.n_must) + rfl(bq.n_must_not);  // behind them only SHOULD terms are left
  const uint32_t n_must = rfl(bq.n_must);
  const BoolTerm *const row = p.terms + ((size_t)rfl(bq.term_begin) * p.n_segs + (size_t)seg * nt);
  const SegDev sd = bool_load_const(p.segs + seg);
  const gdoc_t docs = (gdoc_t)sd.docs;
  const uint32_t ccnt = rfl(bool_load_const(p.slice_ccnt + s));
  const uint64_t cb = bool_load_const(p.slice_cbeg + s);
  uint2 *const reg = p.cand + (((uint64_t)rfl((uint32_t)(cb >> 32)) << 32) | rfl((uint32_t)cb));

  uint32_t kept = 0, rejected = 0;
  for (uint32_t base = 0; base < ccnt; base += 64u) {
    const uint32_t i = base + lane;
    uint2 c = make_uint2(0u, 0xFFFFFFFFu);
    if (i < ccnt) c = reg[i];
    const uint32_t doc = c.y;
    const bool live = doc != 0xFFFFFFFFu;  // (a dropped entry stays dropped and is nobody's reject)
    uint32_t held = 0;
    bool open = live;  // not decided yet: this lane still probes
    for (uint32_t ti = 0; ti < nt; ti += G) {
      uint64_t off[G];
      uint32_t n[G], grp[G], pos[G];
#pragma unroll
      for (int g = 0; g < G; g++) {
        const BoolTerm t = bool_load_const(row + (ti + g < nt ? ti + g : ti));
        off[g] = ((uint64_t)rfl((uint32_t)(t.off >> 32)) << 32) | rfl((uint32_t)t.off);
        n[g] = ti + g < nt ? rfl(t.df) : 0u;  // (uniform: the lanes of a wave search the same lists)
        grp[g] = rfl(t.group);
        pos[g] = 0u;
      }
      // the last posting <= doc of each list (or posting 0): every probe lies in [off, off + df)
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
      // decided: rejected for good (a MUST_NOT group holds the doc; every MUST term was searched and a MUST
      // group does not), or accepted for good (only SHOULD terms are left and enough SHOULD groups hold it)
      const uint32_t done = ti + G;
      const bool must_ok = (held & must) == must;
      const bool lost = (held & must_not) != 0u || (done >= n_must && !must_ok);
      const bool won = done >= n_rej_terms && must_ok && (uint32_t)__popc(held & should) >= min_should;
      open = open && !lost && !won;
      if (__ballot(open) == 0ull) break;
    }
    const bool accept = live && (held & must) == must && (held & must_not) == 0u &&
                        (uint32_t)__popc(held & should) >= min_should;
    const uint64_t m = __ballot(accept);
    const uint32_t at = kept + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    // IN PLACE: the survivors go back into the same region from its start.  kept <= base, so a chunk's writes
    // land at or before the chunk's own first slot plus the lane's rank among the survivors, i.e. at or before
    // the slot the lane read: a wave working front to back never overwrites a candidate it has not read (every
    // lane of the chunk holds its candidate in registers before the first store, the accept ballot above).
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
