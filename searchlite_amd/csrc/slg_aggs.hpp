// slg_aggs.hpp — the aggregation kernel (slg_batch_prepare_aggs; query/aggs/mod.rs terms, histogram, range
// and stats collectors).  An aggregation batch is planned as a sorted batch: its scoring kernel leaves every
// matched doc of every sub-query in the candidate region, once.  After the batch's select kernel one
// workgroup per query walks the query's slices as select_sorted_kernel does, applies accept() again (the
// reject bitmap: one word per candidate, so the kernel does not depend on what the select left behind), and
// adds every accepted doc to the query's dense tables:
//   counts  u32 [count_cells]   the bucket nodes' tables, node after node, each parent_rows x rows
//   stats   AggStatDev [stats_cells]   the stats nodes' tables, each parent_rows x 1
// A query's tables belong to one workgroup, so nothing has to be visible across workgroups.  Two homes:
//   LDS     4 * count_cells + 32 * stats_cells <= kAggLdsBytes: filled with LDS atomics (u32 add, u64 max on
//           order-preserving keys, f64 add), written out once with plain stores;
//   global  larger tables: the query's slice of the batch's tables, zeroed by a memset on the batch's stream,
//           filled with global atomics of this one workgroup.
// "Distinct per doc" (a doc holding a keyword twice, or two values in one histogram bucket, counts once) is
// a loop over the doc's earlier values: the reference's columns hold a handful of values per doc.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_desc.hpp"
#include "slg_wave.hpp"

namespace slg {

constexpr uint32_t kAggThreads = 256;
constexpr uint32_t kAggLdsBytes = 32768;  // SLG_AGG_LDS_BYTES: five workgroups (20 waves) per CU within 160 KB
constexpr uint32_t kAggMaxRanges = 16;    // SLG_MAX_AGG_RANGES
enum : int32_t { kAggTerms = 0, kAggHistogram = 1, kAggRange = 2, kAggStats = 3 };

// min and max as u64 keys under atomicMax, so that an all-zero cell is the empty one: max_key = the value's
// order-preserving key, min_key = its complement (keys of finite values are neither 0 nor ~0)
struct AggStatDev {
  unsigned long long count, min_key, max_key;
  double sum;
};

struct AggNodeDev {
  int32_t kind, parent;
  uint32_t col;     // the node's column of segment s: cols[col * n_segs + s]
  uint32_t rows;    // rows of the node's table (per parent row)
  uint32_t n_ords;  // terms: real ordinals (rows - 1 when the missing key has a row of its own)
  uint32_t has_missing, missing_ord, has_hard, n_ranges;
  uint32_t off;     // first cell of the node's table in counts (bucket kinds) / stats
  long long first_id;
  double missing, interval, offset, hard_min, hard_max;
  double from[kAggMaxRanges], to[kAggMaxRanges];
};

struct AggParams {
  const QueryRef *queries;
  const uint32_t *slice_seg;
  const uint64_t *slice_cbeg;
  const uint32_t *slice_ccnt;
  const uint2 *cand;  // .x ordered score, .y doc (0xFFFFFFFF: dropped)
  const SegDev *segs;
  const uint32_t *q_filter;             // [nq] 0 = none, f + 1
  const uint32_t *const *reject_table;  // [n_filters * n_segs] reject bitmaps
  const AggNodeDev *nodes;              // [n_nodes]
  const ColumnDev *cols;                // [n_nodes * n_segs]
  uint32_t n_segs, n_nodes, nq;
  uint32_t count_cells, stats_cells;
  uint32_t *counts;                 // [nq * count_cells]
  AggStatDev *stats;                // [nq * stats_cells]
  unsigned long long *out_matched;  // [nq] accepted docs, or null (a sorted batch's select wrote them)
};

__device__ __forceinline__ unsigned long long agg_f64_key(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// One node's collector for one doc; cell = the first cell of the table row the doc goes to (the node's own
// table for a root, the parent bucket's row of it for a child).  child(b): the doc was counted in bucket b.
template <typename F>
__device__ __forceinline__ void agg_collect(const AggParams &p, const AggNodeDev &n, const uint32_t seg,
                                            const uint32_t doc, const uint32_t cell, uint32_t *cnt, AggStatDev *st,
                                            F &&child) {
  const ColumnDev col = p.cols[(size_t)n.col * p.n_segs + seg];
  uint32_t a, e;
  column_range(col, doc, a, e);
  if (n.kind == kAggTerms) {
    const uint32_t *v = col.ords();
    if (e == a) {
      if (n.has_missing && n.missing_ord < n.rows) {
        atomicAdd(&cnt[cell + n.missing_ord], 1u);
        child(n.missing_ord);
      }
      return;
    }
    for (uint32_t i = a; i < e; i++) {
      const uint32_t o = v[i];
      if (o >= n.n_ords) continue;  // (registration refuses such a column)
      bool dup = false;
      for (uint32_t j = a; j < i; j++) dup = dup || v[j] == o;
      if (dup) continue;
      atomicAdd(&cnt[cell + o], 1u);
      child(o);
    }
    return;
  }
  const double *v = col.f64();
  const bool miss = e == a;
  if (miss && !n.has_missing) return;
  const uint32_t nv = miss ? 1u : e - a;
  auto val = [&](const uint32_t i) { return miss ? n.missing : v[a + i]; };
  if (n.kind == kAggStats) {
    AggStatDev *s = st + cell;
    for (uint32_t i = 0; i < nv; i++) {
      const double x = val(i);
      const unsigned long long key = agg_f64_key(x);
      atomicAdd(&s->count, 1ull);
      atomicMax(&s->min_key, ~key);
      atomicMax(&s->max_key, key);
      unsafeAtomicAdd(&s->sum, x);  // (the hardware's f64 add, LDS or device memory: no compare-and-swap loop)
    }
    return;
  }
  if (n.kind == kAggHistogram) {
    // id = floor((val - offset) / interval): IEEE f64 subtraction, division and floor (no fast-math, no fma)
    auto bucket = [&](const double x, long long &id) {
      if (n.has_hard && (x < n.hard_min || x > n.hard_max)) return false;
      id = (long long)floor((x - n.offset) / n.interval);
      return true;
    };
    for (uint32_t i = 0; i < nv; i++) {
      long long id = 0;
      if (!bucket(val(i), id)) continue;
      bool dup = false;
      for (uint32_t j = 0; j < i; j++) {
        long long jd = 0;
        dup = dup || (bucket(val(j), jd) && jd == id);
      }
      const long long row = id - n.first_id;
      if (dup || row < 0 || row >= (long long)n.rows) continue;  // (outside: the host's range covers every value)
      atomicAdd(&cnt[cell + (uint32_t)row], 1u);
      child((uint32_t)row);
    }
    return;
  }
  // kAggRange: once in every range that holds any of the doc's values (`to` inclusive)
  for (uint32_t r = 0; r < n.n_ranges && r < n.rows; r++) {
    bool in = false;
    for (uint32_t i = 0; i < nv; i++) {
      const double x = val(i);
      in = in || (x >= n.from[r] && x <= n.to[r]);
    }
    if (!in) continue;
    atomicAdd(&cnt[cell + r], 1u);
    child(r);
  }
}

template <bool LDS>
static __global__ void __launch_bounds__(kAggThreads) agg_kernel(AggParams p) {
  extern __shared__ unsigned long long agg_lds[];  // (LDS) the stats cells, then the count cells
  __shared__ uint32_t sh_matched;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t q = blockIdx.x;
  if (q >= p.nq) return;
  const QueryRef qr = p.queries[q];
  const uint32_t sb = qr.slice_begin, se = qr.slice_end;
  const uint32_t flt = p.q_filter ? p.q_filter[q] : 0u;
  AggStatDev *st = LDS ? reinterpret_cast<AggStatDev *>(agg_lds) : p.stats + (size_t)q * p.stats_cells;
  uint32_t *cnt = LDS ? reinterpret_cast<uint32_t *>(agg_lds + 4 * (size_t)p.stats_cells)
                      : p.counts + (size_t)q * p.count_cells;
  if (tid == 0) sh_matched = 0;
  if (LDS) {
    const uint32_t words = 8 * p.stats_cells + p.count_cells;  // every cell starts as zero words
    uint32_t *w = reinterpret_cast<uint32_t *>(agg_lds);
    for (uint32_t i = tid; i < words; i += kAggThreads) w[i] = 0u;
  }
  __syncthreads();

  uint32_t nv = 0;
  for (uint32_t s = sb + wave; s < se; s += kAggThreads / 64) {  // a wave per slice, as the selects
    const uint64_t base = p.slice_cbeg[s];
    const uint32_t n = p.slice_ccnt[s];
    const uint32_t seg = p.slice_seg[s];
    const uint32_t *del = flt ? p.reject_table[(size_t)(flt - 1) * p.n_segs + seg] : p.segs[seg].deleted;
    for (uint32_t i = lane; i < n; i += 64) {
      const uint32_t doc = p.cand[base + i].y;
      if (doc == 0xFFFFFFFFu) continue;
      if (del && ((del[doc >> 5] >> (doc & 31)) & 1u)) continue;
      nv++;
      for (uint32_t r = 0; r < p.n_nodes; r++) {
        const AggNodeDev &root = p.nodes[r];
        if (root.parent >= 0) continue;
        agg_collect(p, root, seg, doc, root.off, cnt, st, [&](const uint32_t b) {
          for (uint32_t c = r + 1; c < p.n_nodes; c++) {
            const AggNodeDev &ch = p.nodes[c];
            if (ch.parent != (int32_t)r) continue;
            agg_collect(p, ch, seg, doc, ch.off + b * ch.rows, cnt, st, [](uint32_t) {});
          }
        });
      }
    }
  }
  nv = wave_sum(nv);
  if (lane == 0 && nv) atomicAdd(&sh_matched, nv);
  __syncthreads();
  if (tid == 0 && p.out_matched) p.out_matched[q] = sh_matched;
  if (LDS) {
    uint32_t *oc = p.counts + (size_t)q * p.count_cells;
    for (uint32_t i = tid; i < p.count_cells; i += kAggThreads) oc[i] = cnt[i];
    unsigned long long *os = reinterpret_cast<unsigned long long *>(p.stats + (size_t)q * p.stats_cells);
    for (uint32_t i = tid; i < 4 * p.stats_cells; i += kAggThreads) os[i] = agg_lds[i];
  }
}

}  // namespace slg
