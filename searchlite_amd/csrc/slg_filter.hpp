// slg_filter.hpp — filter_tree_kernel: a filter tree (query/filters.rs:84-149) over the registered aggregation
// columns, evaluated doc by doc into the reject bitmap every batch kind reads (slg_index_add_filter_trees).  Only
// slg_index.hip includes it, beside slg_stage.hpp (a static kernel is compiled into every unit that includes its
// header).  The image the kernel reads is planned on the host (slg_plan.cpp: plan_filter_trees).
//
// One doc per lane, one wave per 64 consecutive docs (two whole reject words), blockIdx.y = the tree.  The program
// is the same for every lane: the node rows are read with scalar loads (load_const), so a node's kind and arity
// steer scalar branches and only the column walks diverge.  A lane's evaluation stack is the bits of one word
// (bit 0 = top; the host refuses a program that would go deeper than kFilterMaxDepth).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_desc.hpp"
#include "slg_wave.hpp"

namespace slg {

struct FilterTreeParams {
  const FilterTreeDev *trees;            // [gridDim.y]
  const FilterNodeDev *nodes;
  const ColumnDev *cols;                 // [column rows][n_segs]
  const uint32_t *const *filters;        // [filter rows][n_segs] reject bitmaps of FILTER_ID leaves
  const uint32_t *words;                 // the ordinal bit sets
  uint32_t *const *out;                  // [gridDim.y][n_segs] the reject bitmaps to write
  const uint32_t *deleted;               // this segment's tombstones, or nullptr
  uint32_t n_docs, seg, n_segs;
};

constexpr uint32_t kFilterThreads = 256;

static __global__ void __launch_bounds__(kFilterThreads) filter_tree_kernel(FilterTreeParams p) {
  const uint32_t d = blockIdx.x * kFilterThreads + threadIdx.x;  // one doc per lane
  const uint32_t lane = threadIdx.x & 63u;
  const bool in = d < p.n_docs;
  const FilterTreeDev t = load_const(p.trees + blockIdx.y);
  const size_t at = (size_t)p.seg;
  uint32_t stack = 0;
  for (uint32_t i = 0; i < t.n_nodes; i++) {
    const FilterNodeDev n = load_const(p.nodes + t.node_begin + i);
    if (n.kind <= kFilterRangeI64) {
      // a leaf over a column: the doc's values are vals[a .. b) (no offsets: exactly vals[d]); a lane past
      // n_docs has none.  The walk ends when no lane of the wave has a value left; a lane that passed stops
      const ColumnDev c = load_const(p.cols + (size_t)n.row * p.n_segs + at);
      uint32_t a = 0, b = 0;
      // (column_range written out: through the helper the kernel takes 18 VGPRs, not 16)
      if (in) {
        a = c.offs ? c.offs[d] : d;
        b = c.offs ? c.offs[d + 1] : d + 1u;
      }
      bool pass = false;
      if (n.kind == kFilterKeywordIn) {
        const uint32_t *ords = c.ords();
        const uint32_t *set = p.words + n.bits;
        while (__ballot(a < b) != 0ull) {
          if (a < b) {
            const uint32_t o = ords[a];
            pass = ((set[o >> 5] >> (o & 31u)) & 1u) != 0u;
            a = pass ? b : a + 1u;
          }
        }
      } else {
        while (__ballot(a < b) != 0ull) {
          if (a < b) {
            const double v = c.f64()[a];
            pass = n.lo <= v && v <= n.hi;  // (a NaN never passes)
            a = pass ? b : a + 1u;
          }
        }
      }
      stack = (stack << 1) | (pass ? 1u : 0u);
    } else if (n.kind == kFilterId) {
      const uint32_t *rej = load_const(p.filters + (size_t)n.row * p.n_segs + at);
      const bool pass = in && ((rej[d >> 5] >> (d & 31u)) & 1u) == 0u;
      stack = (stack << 1) | (pass ? 1u : 0u);
    } else if (n.kind == kFilterNot) {
      stack ^= 1u;
    } else {  // AND / OR over the arity values on top (arity <= kFilterMaxDepth)
      const uint32_t mask = (1u << n.arity) - 1u;
      const bool v = n.kind == kFilterAnd ? (stack & mask) == mask : (stack & mask) != 0u;
      stack = ((stack >> n.arity) << 1) | (v ? 1u : 0u);
    }
  }
  // reject = deleted | ~tree; docs past n_docs are rejected too.  Lanes 0 and 32 store the wave's two words (the
  // second one may lie past the bitmap)
  const uint64_t rej = ~__ballot(in && (stack & 1u) != 0u);
  const uint32_t w = d >> 5, n_words = (p.n_docs + 31u) >> 5;
  if ((lane & 31u) == 0u && w < n_words) {
    uint32_t *out = load_const(p.out + (size_t)blockIdx.y * p.n_segs + at);
    const uint32_t dead = p.deleted ? p.deleted[w] : 0u;
    out[w] = (lane == 0u ? (uint32_t)rej : (uint32_t)(rej >> 32)) | dead;
  }
}

}  // namespace slg
