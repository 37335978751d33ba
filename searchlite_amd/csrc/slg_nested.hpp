// slg_nested.hpp — nested_filter_kernel: filter trees with Nested nodes (query/filters.rs:13-188 over
// index/fastfields.rs:802-907), evaluated into the reject bitmap every batch kind reads
// (slg_index_add_nested_filter_trees).  Only slg_index.hip includes it, beside slg_filter.hpp.  The image the
// kernel reads is planned on the host (slg_plan.cpp: plan_nested_filter_trees).
//
// A tree is evaluated level by level, deepest scopes first, one launch per level and segment, blockIdx.y = the
// scope within the level.  An OBJECT scope (kDocLevel false) runs one lane per object of its path: the lane finds
// its doc through the object -> doc table and its index within the doc by subtracting the doc's first object.  The
// wave writes two words of the scope's object bitmap (PASS bits; a lane past the last object passes nothing).  The
// DOC level (kDocLevel true) runs one lane per doc, as filter_tree_kernel does, and writes the reject bitmap.
// A NESTED leaf is a gather: the lane walks the child scope's bits of its own doc's object range (doc level: whole
// words) and, inside an object scope, keeps the children whose parent is the lane's own object.  No lane writes what
// another reads within one launch, so there is no atomic and no barrier.
//
// As in filter_tree_kernel the program is the same for every lane of a block (node rows through load_const, scalar
// branches on kind and arity, the stack is the bits of one word), and every value walk ends on a ballot.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_desc.hpp"
#include "slg_wave.hpp"

namespace slg {

struct NestedFilterParams {
  const NestedScopeDev *scopes;          // the scope rows; this launch runs scopes[first_scope + blockIdx.y]
  const FilterNodeDev *nodes;
  const ColumnDev *cols;                 // [column rows][n_segs] (doc level)
  const uint32_t *const *filters;        // [filter rows][n_segs] reject bitmaps of FILTER_ID leaves (doc level)
  const uint32_t *words;                 // the ordinal bit sets
  const NestedPathDev *paths;            // [path rows][n_segs]
  const NestedColDev *ncols;             // [nested column rows][n_segs]
  uint32_t *const *obj_bits;             // [object scope rows][n_segs] the pass bits of the scopes' objects
  uint32_t *const *out;                  // [gridDim.y][n_segs] the reject bitmaps to write (doc level)
  const uint32_t *deleted;               // this segment's tombstones, or nullptr
  uint32_t n_docs, seg, n_segs, first_scope;
};

template <bool kDocLevel>
static __global__ void __launch_bounds__(kFilterThreads) nested_filter_kernel(NestedFilterParams p) {
  const uint32_t x = blockIdx.x * kFilterThreads + threadIdx.x;  // one doc / one object per lane
  const uint32_t lane = threadIdx.x & 63u;
  const NestedScopeDev sc = load_const(p.scopes + p.first_scope + blockIdx.y);
  const size_t at = (size_t)p.seg;
  uint32_t d = x, idx = 0, n = p.n_docs;
  if (!kDocLevel) {
    const NestedPathDev own = load_const(p.paths + (size_t)sc.path_row * p.n_segs + at);
    n = own.n_objects;
    if ((x & ~63u) >= n) return;  // (wave-uniform: a level's grid covers its largest scope)
    d = 0;
    if (x < n) {
      d = own.obj_doc[x];
      idx = x - own.base[d];
    }
  }
  const bool in = x < n;
  uint32_t stack = 0;
  for (uint32_t i = 0; i < sc.n_nodes; i++) {
    const FilterNodeDev nd = load_const(p.nodes + sc.node_begin + i);
    if (nd.kind <= kFilterRangeI64) {
      // a leaf over a column: the values of the doc (of the doc's object idx) are vals[a .. b); a lane past the
      // end has none.  The walk ends when no lane of the wave has a value left; a lane that passed stops
      uint32_t a = 0, b = 0;
      const void *vals;
      if (kDocLevel) {
        const ColumnDev c = load_const(p.cols + (size_t)nd.row * p.n_segs + at);
        vals = c.vals;
        if (in) {
          a = c.offs ? c.offs[d] : d;
          b = c.offs ? c.offs[d + 1] : d + 1u;
        }
      } else {
        // the column may hold fewer objects for the doc than the path counts: such an object has no value
        const NestedColDev c = load_const(p.ncols + (size_t)nd.row * p.n_segs + at);
        vals = c.vals;
        if (in && c.doc_offs != nullptr) {
          const uint32_t o0 = c.doc_offs[d];
          if (idx < c.doc_offs[d + 1] - o0) {
            a = c.obj_offs[o0 + idx];
            b = c.obj_offs[o0 + idx + 1u];
          }
        }
      }
      bool pass = false;
      if (nd.kind == kFilterKeywordIn) {
        const uint32_t *ords = static_cast<const uint32_t *>(vals);
        const uint32_t *set = p.words + nd.bits;
        while (__ballot(a < b) != 0ull) {
          if (a < b) {
            const uint32_t o = ords[a];
            pass = ((set[o >> 5] >> (o & 31u)) & 1u) != 0u;
            a = pass ? b : a + 1u;
          }
        }
      } else if (!kDocLevel && nd.kind == kFilterRangeI64) {
        const long long lo = __double_as_longlong(nd.lo), hi = __double_as_longlong(nd.hi);
        while (__ballot(a < b) != 0ull) {
          if (a < b) {
            const long long v = static_cast<const long long *>(vals)[a];
            pass = lo <= v && v <= hi;
            a = pass ? b : a + 1u;
          }
        }
      } else {
        while (__ballot(a < b) != 0ull) {
          if (a < b) {
            const double v = static_cast<const double *>(vals)[a];
            pass = nd.lo <= v && v <= nd.hi;  // (a NaN never passes)
            a = pass ? b : a + 1u;
          }
        }
      }
      stack = (stack << 1) | (pass ? 1u : 0u);
    } else if (nd.kind == kFilterNested) {
      // SOME object of the child scope's path in this doc passed the child scope (its bit is set).  Inside an
      // object scope only the children bound to this object count
      const NestedScopeDev child = load_const(p.scopes + nd.row);
      const NestedPathDev cp = load_const(p.paths + (size_t)child.path_row * p.n_segs + at);
      const uint32_t *bits = load_const(p.obj_bits + (size_t)nd.row * p.n_segs + at);
      uint32_t a = 0, b = 0;
      if (in) {
        a = cp.base[d];
        b = cp.base[d + 1];
      }
      bool pass = false;
      if (kDocLevel) {
        while (__ballot(a < b) != 0ull) {
          if (a < b) {  // the bits a .. min(b, the word's end) of one word
            const bool last = b - 1u <= (a | 31u);  // (compared through b - 1: (a | 31) + 1 may wrap to 0)
            const uint32_t end = (a | 31u) + 1u;
            uint32_t m = ~0u << (a & 31u);
            if (last && (b & 31u) != 0u) m &= (1u << (b & 31u)) - 1u;
            pass = (bits[a >> 5] & m) != 0u;
            a = (pass || last) ? b : end;
          }
        }
      } else {
        // parents.get(j) == Some(idx): the child's entry exists in its doc's parent list and names this object
        uint32_t pa = 0, pn = 0;
        if (in && cp.par_offs != nullptr) {
          pa = cp.par_offs[d];
          pn = cp.par_offs[d + 1] - pa;
        }
        const uint32_t first = a;
        if (pn < b - a) b = a + pn;  // (children past the parent list never bind)
        while (__ballot(a < b) != 0ull) {
          if (a < b) {
            pass = ((bits[a >> 5] >> (a & 31u)) & 1u) != 0u && cp.parents[pa + (a - first)] == idx;
            a = pass ? b : a + 1u;
          }
        }
      }
      stack = (stack << 1) | (pass ? 1u : 0u);
    } else if (kDocLevel && nd.kind == kFilterId) {
      const uint32_t *rej = load_const(p.filters + (size_t)nd.row * p.n_segs + at);
      const bool pass = in && ((rej[d >> 5] >> (d & 31u)) & 1u) == 0u;
      stack = (stack << 1) | (pass ? 1u : 0u);
    } else if (nd.kind == kFilterNot) {
      stack ^= 1u;
    } else {  // AND / OR over the arity values on top (arity <= kFilterMaxDepth)
      const uint32_t mask = (1u << nd.arity) - 1u;
      const bool v = nd.kind == kFilterAnd ? (stack & mask) == mask : (stack & mask) != 0u;
      stack = ((stack >> nd.arity) << 1) | (v ? 1u : 0u);
    }
  }
  // lanes 0 and 32 store the wave's two words (the second one may lie past the bitmap).  Object scope: the pass
  // bits.  Doc level: reject = deleted | ~tree; docs past n_docs are rejected too
  const uint64_t pass = __ballot(in && (stack & 1u) != 0u);
  const uint32_t w = x >> 5, n_words = (uint32_t)(((uint64_t)n + 31u) >> 5);
  if ((lane & 31u) == 0u && w < n_words) {
    const uint32_t mine = lane == 0u ? (uint32_t)pass : (uint32_t)(pass >> 32);
    if (kDocLevel) {
      uint32_t *out = load_const(p.out + (size_t)blockIdx.y * p.n_segs + at);
      out[w] = ~mine | (p.deleted ? p.deleted[w] : 0u);
    } else {
      uint32_t *out = load_const(p.obj_bits + (size_t)(p.first_scope + blockIdx.y) * p.n_segs + at);
      out[w] = mine;
    }
  }
}

}  // namespace slg
