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
// The kernel is built from the clause-filter core it shares with phrase_filter_kernel (slg_clause.hpp): the
// slice prologue, then per chunk of 64 candidates the pass over the query's term groups and the in-place store
// of the survivors, then the slice's new count.  The term-group pass alone is written out here: as a call of
// clause_term_pass the same loop costs this kernel two vector registers (18 against 16; the phrase kernel keeps
// its 42 with the shared pass), so this is the one copy of it that stays — a change to clause_term_pass or
// clause_search (the invariants are stated there) belongs here too.
#pragma once

#include "slg_clause.hpp"

namespace slg {

constexpr int kBoolThreads = 256;  // four waves = four slices per workgroup

static __global__ void __launch_bounds__(kBoolThreads) bool_filter_kernel(BoolFilterParams p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = rfl(blockIdx.x * (kBoolThreads / 64) + (threadIdx.x >> 6));
  if (s >= p.n_slices) return;
  ClauseSlice sl = clause_query(p, s);
  if (sl.nt == 0u) return;  // a query without a clause table is left as it is
  clause_region(p, s, sl);
  constexpr int G = kClauseListsPerStep;
  for (uint32_t base = 0; base < sl.ccnt; base += 64u) {
    const uint2 c = clause_candidate(sl, base + lane);
    const bool live = c.y != 0xFFFFFFFFu;  // (a dropped entry stays dropped)
    const uint32_t doc = c.y;
    uint32_t held = 0;
    bool open = live;  // not decided yet: this lane still probes
    for (uint32_t ti = 0; ti < sl.nt; ti += G) {
      uint64_t off[G];
      uint32_t n[G], grp[G], pos[G];
#pragma unroll
      for (int g = 0; g < G; g++) {
        const BoolTerm t = load_const(sl.row + (ti + g < sl.nt ? ti + g : ti));
        off[g] = uniform64(t.off);
        n[g] = ti + g < sl.nt ? rfl(t.df) : 0u;  // (uniform: the lanes of a wave search the same lists)
        grp[g] = rfl(t.group);
        pos[g] = 0u;
      }
      // clause_search<G>, written out
      bool more = false;
#pragma unroll
      for (int g = 0; g < G; g++) more = more || n[g] > 1u;
      while (more) {
        uint32_t v[G], half[G];
#pragma unroll
        for (int g = 0; g < G; g++) {
          half[g] = n[g] >> 1;
          v[g] = 0xFFFFFFFFu;
          if (n[g] > 1u && open) v[g] = sl.docs[off[g] + pos[g] + half[g]];
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
        if (n[g] != 0u && open) hit_doc[g] = sl.docs[off[g] + pos[g]];
      }
#pragma unroll
      for (int g = 0; g < G; g++)
        if (open && hit_doc[g] == doc) held |= 1u << grp[g];
      // decided: rejected for good (a MUST_NOT group holds the doc; every MUST term was searched and a MUST
      // group does not), or accepted for good (only SHOULD terms are left and enough SHOULD groups hold it)
      const uint32_t done = ti + G;
      const bool must_ok = (held & sl.must) == sl.must;
      const bool lost = (held & sl.must_not) != 0u || (done >= sl.n_must && !must_ok);
      const bool won = done >= sl.n_rej_terms && must_ok && (uint32_t)__popc(held & sl.should) >= sl.min_should;
      open = open && !lost && !won;
      if (__ballot(open) == 0ull) break;
    }
    clause_keep(sl, c, live, clause_accepts(sl, held, live));
  }
  clause_finish(p, s, sl, lane);
}

}  // namespace slg
