// slg_booltree.hpp — nested boolean matchers (slg_batch_prepare_bool_tree): the reference's matcher TREE
// (QueryEvaluator::matches_node, api/reader.rs:1485-1565: a Bool may hold Bool, DisMax, QueryString and MatchAll
// children and a filter list of its own) as one kernel between the scoring kernel and the select, in
// bool_filter_kernel's place.  The semantics in full: include/searchlite_gpu.h; the tables: slg_desc.hpp.
//
// Shape: the clause filters' (slg_clause.hpp, whose helpers are used as they are) — one wave per slice, four per
// workgroup, one candidate per lane, 64 per chunk; the query's record, its nodes, its filter rows and the
// (query, segment) row of BoolTerms are wave-uniform and read through the constant address space.  Per lane: the
// two value masks t and f (slg_desc.hpp, booltree_eval) and the registers of four binary searches.  No LDS.
//
// Per chunk: the filter leaves first (one word of a reject bitmap per leaf and lane: known from the start), then
// the term row in steps of four lists searched side by side.  The wave keeps the uniform mask `known` of the
// leaves whose every term has been searched (a term with df 0 costs no load), and after every step runs
// booltree_eval over what is known: a lane whose root is decided either way takes that verdict and stops probing,
// and a ballot ends the row when no lane is open.  Once every leaf is known the root is decided, so a lane that is
// still open behind the row's last step gets its verdict from the same pass.
#pragma once

#include "slg_clause.hpp"

namespace slg {

constexpr int kBoolTreeThreads = 256;  // four waves = four slices per workgroup

struct BoolTreeParams {
  BoolFilterParams c;              // the slices, the candidates, q_scored and the BoolTerm rows (queries: unused, null)
  const BoolTreeQuery *queries;    // [nq]
  const BoolTreeNode *nodes;       // the nodes of all queries
  const uint32_t *filt_rows;       // the filter leaves of all queries: their rows of `filters`
  const uint32_t *const *filters;  // [filters of the batch][n_segs] reject bitmaps (bit set: the filter rejects)
};

static __global__ void __launch_bounds__(kBoolTreeThreads) booltree_filter_kernel(BoolTreeParams p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = rfl(blockIdx.x * (kBoolTreeThreads / 64) + (threadIdx.x >> 6));
  if (s >= p.c.n_slices) return;
  const RoundQuery rq = load_const(p.c.sq + load_const(p.c.slice_sq + s));
  ClauseSlice sl;
  sl.q = rfl(rq.q);
  sl.seg = rfl(rq.seg);
  const BoolTreeQuery tq = load_const(p.queries + sl.q);
  const uint32_t n_nodes = rfl(tq.n_nodes);
  if (n_nodes == 0u) return;  // a query without a matcher is left as it is
  sl.nt = rfl(tq.n_terms);
  sl.row = p.c.terms + ((size_t)rfl(tq.term_begin) * p.c.n_segs + (size_t)sl.seg * sl.nt);
  sl.kept = sl.rejected = 0u;
  clause_region(p.c, s, sl);
  const BoolTreeNode *const nodes = p.nodes + rfl(tq.node_begin);
  const auto node_at = [nodes](uint32_t i) {
    BoolTreeNode n = load_const(nodes + i);
    n.must = uniform64(n.must);
    n.must_not = uniform64(n.must_not);
    n.should = uniform64(n.should);
    n.min_should = rfl(n.min_should);
    return n;
  };
  const uint64_t root = 1ull << (31u + n_nodes);
  const uint32_t n_filters = rfl(tq.n_filters);
  const uint32_t first_filter = rfl(tq.n_leaves) - n_filters;  // the filter leaves are the query's last leaves
  const uint32_t *const frows = p.filt_rows + rfl(tq.filt_begin);
  const uint64_t known_filters = n_filters ? (((1ull << n_filters) - 1ull) << first_filter) : 0ull;
  constexpr int G = kClauseListsPerStep;
  for (uint32_t base = 0; base < sl.ccnt; base += 64u) {
    const uint2 c = clause_candidate(sl, base + lane);
    const bool live = c.y != 0xFFFFFFFFu;  // (a dropped entry stays dropped)
    const uint32_t doc = c.y;
    uint64_t t = 0ull, f = 0ull;
    for (uint32_t i = 0; i < n_filters; i++) {
      const uint32_t r = rfl(load_const(frows + i));
      const uint64_t a = uniform64((uint64_t)(uintptr_t)load_const(p.filters + ((size_t)r * p.c.n_segs + sl.seg)));
      uint32_t w = 0u;
      if (live && a != 0ull) w = ((clause_gu32_t)(uintptr_t)a)[doc >> 5];  // (a live doc is below the segment's n_docs)
      if (((w >> (doc & 31u)) & 1u) == 0u) t |= 1ull << (first_filter + i);
    }
    uint64_t known = known_filters;  // uniform: the leaves every lane of the chunk knows
    bool open = live, verdict = false;
    // the pass over what is known; a lane that is no longer open keeps the verdict it was decided with (its t
    // misses the leaves it did not probe for)
    const auto decide = [&]() {
      f |= known & ~t;
      booltree_eval(node_at, n_nodes, t, f);
      const bool yes = (t & root) != 0ull, no = (f & root) != 0ull;
      verdict = open ? yes : verdict;
      open = open && !yes && !no;
    };
    decide();
    for (uint32_t ti = 0; ti < sl.nt && __ballot(open) != 0ull; ti += G) {
      uint64_t off[G];
      uint32_t n[G], grp[G], at[G];
      bool hit[G];
#pragma unroll
      for (int g = 0; g < G; g++) {
        const BoolTerm bt = load_const(sl.row + (ti + g < sl.nt ? ti + g : ti));
        off[g] = uniform64(bt.off);
        n[g] = ti + g < sl.nt ? rfl(bt.df) : 0u;  // (uniform: the lanes of a wave search the same lists)
        grp[g] = ti + g < sl.nt ? rfl(bt.group) : 0u;
      }
      clause_search<G>(off, n, sl.docs, doc, open, at, hit);
#pragma unroll
      for (int g = 0; g < G; g++) {
        if (hit[g]) t |= 1ull << (grp[g] & 31u);
        if (grp[g] & kBoolTreeLeafEnd) known |= 1ull << (grp[g] & 31u);  // (a slot behind the row: group 0, no end)
      }
      decide();
    }
    clause_keep(sl, c, live, live && verdict);
  }
  clause_finish(p.c, s, sl, lane);
}

}  // namespace slg
