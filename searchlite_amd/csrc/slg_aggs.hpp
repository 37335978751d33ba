// slg_aggs.hpp — the aggregation kernel (slg_batch_prepare_aggs; query/aggs/mod.rs terms, histogram, range,
// date_histogram, filter and stats collectors).  An aggregation batch is planned as a sorted batch: its scoring
// kernel leaves every matched doc of every sub-query in the candidate region, once.  After the batch's select
// kernel one workgroup per query walks the query's slices as select_sorted_kernel does, applies accept() again
// (the reject bitmap: one word per candidate, so the kernel does not depend on what the select left behind),
// and adds every accepted doc to the query's dense tables:
//   counts  u32 [count_cells]   the bucket nodes' tables, node after node, each parent_rows x rows
//   stats   AggStatDev [stats_cells]   the stats nodes' tables, each parent_rows x 1
// A query's tables belong to one workgroup, so nothing has to be visible across workgroups.  Two homes:
//   LDS     4 * count_cells + 32 * stats_cells <= kAggLdsBytes: filled with LDS atomics (u32 add, u64 max on
//           order-preserving keys, f64 add), written out once with plain stores;
//   global  larger tables: the query's slice of the batch's tables, zeroed by a memset on the batch's stream,
//           filled with global atomics of this one workgroup.
// Value nodes (cardinality, percentiles, percentile_ranks) are order and identity questions over the values of
// the matched set: agg_values_kernel, launched behind agg_kernel only when the spec has such a node, answers them
// from the value ranks of the column (slg_index_rank_agg_field): a per-query bitmap over the ranks, counters, and
// a two-pass radix select on the ranks (see the kernel).
// "Distinct per doc" (a doc holding a keyword twice, or two values in one histogram bucket, counts once) is
// a loop over the doc's earlier values: the reference's columns hold a handful of values per doc.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_date.hpp"
#include "slg_desc.hpp"
#include "slg_wave.hpp"

namespace slg {

constexpr uint32_t kAggThreads = 256;
constexpr uint32_t kAggLdsBytes = 32768;  // SLG_AGG_LDS_BYTES: five workgroups (20 waves) per CU within 160 KB
constexpr uint32_t kAggMaxRanges = 16;    // SLG_MAX_AGG_RANGES
constexpr uint32_t kAggPctLdsBytes = 16384;  // SLG_AGG_PCT_LDS_BYTES: a percentiles node's 4096 coarse bins, then its fine tables
constexpr uint32_t kAggCoarseBits = 12;
constexpr uint32_t kAggNoRank = 0xFFFFFFFFu;
enum : int32_t {
  kAggTerms = 0, kAggHistogram = 1, kAggRange = 2, kAggStats = 3,
  kAggCardinality = 4, kAggPercentiles = 5, kAggPercentileRanks = 6,
  kAggDateHistogram = 8, kAggFilter = 9
};

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
  uint32_t off;     // first cell of the node's table in counts (bucket kinds) / stats / values
  long long first_id;
  double missing, interval, offset, hard_min, hard_max;
  double from[kAggMaxRanges], to[kAggMaxRanges];  // (from: the percents / targets of a value node)
  // value nodes.  A value's rank is ranks[i] + (ranks[i] >= shift_from); a doc without a value has miss_rank.
  uint32_t n_ranks;     // ranks the node can see (the virtual rank of `missing` included), >= 1
  uint32_t miss_rank;
  uint32_t shift_from;  // kAggNoRank: no virtual rank (the dictionary holds `missing`, or it lies beyond it)
  uint32_t wpr, bm_off; // cardinality: words of one bitmap row; first word of the node's bitmaps
  uint32_t shift;       // percentiles: coarse bin = rank >> shift
  uint32_t fine_lds, fine_off;  // percentiles: the fine tables lie in LDS, or at this word of the scratch slice
  const double *dict;   // percentiles: the value of every real rank
  // date_histogram: SLG_DATE_*, then i64 milliseconds (has_hard: the two bounds are read); filter: the filter's row
  // of reject_table
  uint32_t unit, filter;
  long long step, date_offset, date_hard_min, date_hard_max;
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

// The accepted candidates of query qr, a wave per slice and a lane per candidate, as the selects walk them.
// CONVERGED: f(ok, seg, doc) runs for ALL lanes of a wave together (ok false: no candidate, a dropped one, a
// tombstone or a doc the filter rejects), so that f may use wave-wide operations; else f runs for the accepted
// candidates only (ok is true).
// (It has a twin: top_hits_walk in slg_tophits.hpp is the CONVERGED form with the candidate's score, slice and position
// in the callback.  What changes here — the slices of a query, the tombstone and filter test — changes there too.)
template <bool CONVERGED, typename P, typename F>
__device__ __forceinline__ void agg_walk(const P &p, const QueryRef &qr, const uint32_t flt, const uint32_t wave,
                                         const uint32_t lane, F &&f) {
  for (uint32_t s = qr.slice_begin + wave; s < qr.slice_end; s += kAggThreads / 64) {
    const uint64_t base = p.slice_cbeg[s];
    const uint32_t n = p.slice_ccnt[s];
    const uint32_t seg = p.slice_seg[s];
    const uint32_t *del = flt ? p.reject_table[(size_t)(flt - 1) * p.n_segs + seg] : p.segs[seg].deleted;
    if (CONVERGED) {
      for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + lane;
        const uint32_t doc = i < n ? p.cand[base + i].y : 0xFFFFFFFFu;
        const bool ok = doc != 0xFFFFFFFFu && !(del && ((del[doc >> 5] >> (doc & 31)) & 1u));
        f(ok, seg, doc);
      }
    } else {
      for (uint32_t i = lane; i < n; i += 64) {
        const uint32_t doc = p.cand[base + i].y;
        if (doc == 0xFFFFFFFFu) continue;
        if (del && ((del[doc >> 5] >> (doc & 31)) & 1u)) continue;
        f(true, seg, doc);
      }
    }
  }
}

// The values of one doc in a numeric node's column: x(i), i < nv (a doc without a value has the one value
// `missing` if the node has one: numeric_values, aggs/mod.rs:597-610)
struct AggDocValues {
  const double *v;
  uint32_t a, nv;
  bool miss;
  double missing;
  __device__ __forceinline__ double x(const uint32_t i) const { return miss ? missing : v[a + i]; }
};
__device__ __forceinline__ AggDocValues agg_doc_values(const AggNodeDev &n, const ColumnDev &col, const uint32_t a,
                                                       const uint32_t e) {
  const bool miss = e == a;
  return AggDocValues{col.f64(), a, miss ? (n.has_missing ? 1u : 0u) : e - a, miss, n.missing};
}
template <typename P>
__device__ __forceinline__ AggDocValues agg_doc_values(const P &p, const AggNodeDev &n, const uint32_t seg,
                                                       const uint32_t doc) {
  const ColumnDev col = p.cols[(size_t)n.col * p.n_segs + seg];
  uint32_t a, e;
  column_range(col, doc, a, e);
  return agg_doc_values(n, col, a, e);
}

// A filter node's one bucket: the doc's bit in the reject bitmap of the node's filter is clear (a segment
// without a bitmap rejects nothing).  A filter node has no column: nothing of `cols` is read for it.
template <typename P>
__device__ __forceinline__ bool agg_filter_passes(const P &p, const AggNodeDev &n, const uint32_t seg,
                                                  const uint32_t doc) {
  const uint32_t *rej = p.reject_table[(size_t)n.filter * p.n_segs + seg];
  return !(rej && ((rej[doc >> 5] >> (doc & 31)) & 1u));
}

// The buckets of bucket node n (not a filter node) that one doc is counted in: emit(row) once per bucket; the
// doc's values in the node's column are [a, e) of col.  Shared by agg_kernel (the node's own counts, and the rows
// its children collect into) and agg_values_kernel (the rows of a value child).  EXT: the spec has a
// date_histogram or filter node; a spec without one runs the instantiation that holds neither path (its registers
// are what they were without them).
template <bool EXT, typename F>
__device__ __forceinline__ void agg_buckets(const AggNodeDev &n, const ColumnDev &col, const uint32_t a,
                                            const uint32_t e, F &&emit) {
  if (n.kind == kAggTerms) {
    const uint32_t *v = col.ords();
    if (e == a) {
      if (n.has_missing && n.missing_ord < n.rows) emit(n.missing_ord);
      return;
    }
    for (uint32_t i = a; i < e; i++) {
      const uint32_t o = v[i];
      if (o >= n.n_ords) continue;  // (registration refuses such a column)
      bool dup = false;
      for (uint32_t j = a; j < i; j++) dup = dup || v[j] == o;
      if (dup) continue;
      emit(o);
    }
    return;
  }
  const AggDocValues d = agg_doc_values(n, col, a, e);
  const bool date = EXT && n.kind == kAggDateHistogram;
  if (n.kind == kAggHistogram || date) {
    // histogram: id = floor((val - offset) / interval): IEEE f64 subtraction, division and floor (no fast-math, no
    // fma).  date_histogram: the value `as i64` (truncated toward zero), i64 hard bounds, date_bucket_id
    auto bucket = [&](const double x, long long &id) {
      if (date) {
        const long long v = (long long)x;
        if (n.has_hard && (v < n.date_hard_min || v > n.date_hard_max)) return false;
        id = date_bucket_id(n.unit, n.step, n.date_offset, v);
        return true;
      }
      if (n.has_hard && (x < n.hard_min || x > n.hard_max)) return false;
      id = (long long)floor((x - n.offset) / n.interval);
      return true;
    };
    for (uint32_t i = 0; i < d.nv; i++) {
      long long id = 0;
      if (!bucket(d.x(i), id)) continue;
      bool dup = false;
      for (uint32_t j = 0; j < i; j++) {
        long long jd = 0;
        dup = dup || (bucket(d.x(j), jd) && jd == id);
      }
      const long long row = id - n.first_id;
      if (dup || row < 0 || row >= (long long)n.rows) continue;  // (outside: the host's range covers every value)
      emit((uint32_t)row);
    }
    return;
  }
  if (n.kind != kAggRange) return;
  // once in every range that holds any of the doc's values (`to` inclusive)
  for (uint32_t r = 0; r < n.n_ranges && r < n.rows; r++) {
    bool in = false;
    for (uint32_t i = 0; i < d.nv; i++) {
      const double x = d.x(i);
      in = in || (x >= n.from[r] && x <= n.to[r]);
    }
    if (in) emit(r);
  }
}
template <bool EXT, typename P, typename F>
__device__ __forceinline__ void agg_buckets(const P &p, const AggNodeDev &n, const uint32_t seg, const uint32_t doc,
                                            F &&emit) {
  if (EXT && n.kind == kAggFilter) {
    if (agg_filter_passes(p, n, seg, doc)) emit(0u);
    return;
  }
  const ColumnDev col = p.cols[(size_t)n.col * p.n_segs + seg];
  uint32_t a, e;
  column_range(col, doc, a, e);
  agg_buckets<EXT>(n, col, a, e, emit);
}


// One node's collector for one doc; cell = the first cell of the table row the doc goes to (the node's own
// table for a root, the parent bucket's row of it for a child).  child(b): the doc was counted in bucket b.
// (value nodes are agg_values_kernel's)
template <bool EXT, typename F>
__device__ __forceinline__ void agg_collect(const AggParams &p, const AggNodeDev &n, const uint32_t seg,
                                            const uint32_t doc, const uint32_t cell, uint32_t *cnt, AggStatDev *st,
                                            F &&child) {
  if (EXT && n.kind == kAggFilter) {  // (no column)
    if (!agg_filter_passes(p, n, seg, doc)) return;
    atomicAdd(&cnt[cell], 1u);
    child(0u);
    return;
  }
  // (the column and the doc's range are read before the kind decides: the loads go out together)
  const ColumnDev col = p.cols[(size_t)n.col * p.n_segs + seg];
  uint32_t a, e;
  column_range(col, doc, a, e);
  if (n.kind > kAggStats && !(EXT && n.kind == kAggDateHistogram)) return;
  if (n.kind == kAggStats) {
    const AggDocValues d = agg_doc_values(n, col, a, e);
    AggStatDev *s = st + cell;
    for (uint32_t i = 0; i < d.nv; i++) {
      const double x = d.x(i);
      const unsigned long long key = agg_f64_key(x);
      atomicAdd(&s->count, 1ull);
      atomicMax(&s->min_key, ~key);
      atomicMax(&s->max_key, key);
      unsafeAtomicAdd(&s->sum, x);  // (the hardware's f64 add, LDS or device memory: no compare-and-swap loop)
    }
    return;
  }
  agg_buckets<EXT>(n, col, a, e, [&](const uint32_t b) {
    atomicAdd(&cnt[cell + b], 1u);
    child(b);
  });
}

template <bool LDS, bool EXT>
static __global__ void __launch_bounds__(kAggThreads) agg_kernel(AggParams p) {
  extern __shared__ unsigned long long agg_lds[];  // (LDS) the stats cells, then the count cells
  __shared__ uint32_t sh_matched;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t q = blockIdx.x;
  if (q >= p.nq) return;
  const QueryRef qr = p.queries[q];
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
  agg_walk<false>(p, qr, flt, wave, lane, [&](bool, const uint32_t seg, const uint32_t doc) {
    nv++;
    for (uint32_t r = 0; r < p.n_nodes; r++) {
      const AggNodeDev &root = p.nodes[r];
      if (root.parent >= 0) continue;
      agg_collect<EXT>(p, root, seg, doc, root.off, cnt, st, [&](const uint32_t b) {
        for (uint32_t c = r + 1; c < p.n_nodes; c++) {
          const AggNodeDev &ch = p.nodes[c];
          if (ch.parent != (int32_t)r) continue;
          agg_collect<EXT>(p, ch, seg, doc, ch.off + b * ch.rows, cnt, st, [](uint32_t) {});
        }
      });
    }
  });
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

// ---- value nodes --------------------------------------------------------------------------------------
// One workgroup per query, as agg_kernel.  The query's value table is [value_cells] 8-byte cells.  Homes:
//   XLDS   8 * value_cells + 4 * card_words <= kAggLdsBytes - (kAggPctLdsBytes when the spec has a percentiles
//          node): the value cells and the cardinality bitmaps live in LDS (ds_or_b32, ds_add_u64), written out once;
//   else   the value cells are the query's slice of `values` and the bitmaps its slice of `scratch`, both zeroed by
//          a memset on the batch's stream and filled with global atomics of this one workgroup; what the workgroup
//          reads back of them it reads past its L1 (an agent-scope load).
// Walk 1 (when the spec has a cardinality or percentile_ranks node): the bit of every rank of the doc in the row of
// each parent bucket it was counted in; n and the counts of values <= target.  Then a popcount per bitmap row.
// Per percentiles node, a two-pass radix select on the ranks: walk A histograms rank >> shift into at most 4096
// LDS bins; the workgroup prefix-sums them and maps every order statistic (low and high per percent, at most 32)
// to a coarse bin and a residual; walk B (shift > 0 only) histograms the low bits of the ranks that fall in a
// selected bin, into [selected][1 << shift] cells (in the LDS the coarse bins leave behind when they fit, else in
// the scratch slice); a wave per order statistic scans its row.  No compare-and-swap loop anywhere.
struct AggValueParams {
  const QueryRef *queries;
  const uint32_t *slice_seg;
  const uint64_t *slice_cbeg;
  const uint32_t *slice_ccnt;
  const uint2 *cand;
  const SegDev *segs;
  const uint32_t *q_filter;
  const uint32_t *const *reject_table;
  const AggNodeDev *nodes;             // [n_nodes]
  const ColumnDev *cols;               // [n_nodes * n_segs]
  const uint32_t *const *rank_cols;    // [n_nodes * n_segs] the ranks beside a column's values (keyword: the ordinals)
  uint32_t n_segs, n_nodes, nq;
  uint32_t value_cells, card_words;    // of one query
  uint32_t pct_words;                  // LDS words in front of the X region (0 or kAggPctLdsBytes / 4)
  uint32_t scratch_words;              // of one query's slice of scratch
  uint32_t walk1;                      // the spec has a cardinality or percentile_ranks node
  unsigned long long *values;          // [nq * value_cells]
  uint32_t *scratch;                   // [nq * scratch_words]
};

template <bool G>
__device__ __forceinline__ uint32_t agg_read_back(const uint32_t *w) {
  return G ? __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *w;
}

// the value of rank r of a percentiles node
__device__ __forceinline__ double agg_rank_value(const AggNodeDev &n, uint32_t r) {
  if (n.shift_from != kAggNoRank) {
    if (r == n.shift_from) return n.missing;
    if (r > n.shift_from) r--;
  }
  return n.dict[r];
}

template <bool XLDS, bool EXT>
static __global__ void __launch_bounds__(kAggThreads) agg_values_kernel(AggValueParams p) {
  extern __shared__ unsigned long long av_lds[];  // the percentiles region, then (XLDS) value cells and bitmaps
  __shared__ uint32_t sh_wtot[kAggThreads / 64], sh_n, sh_nsel;
  __shared__ uint32_t sh_kbin[2 * kAggMaxRanges], sh_kres[2 * kAggMaxRanges], sh_ksel[2 * kAggMaxRanges];
  __shared__ uint32_t sh_selbin[2 * kAggMaxRanges], sh_selmap[(1u << kAggCoarseBits) / 32];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t q = blockIdx.x;
  if (q >= p.nq) return;
  const QueryRef qr = p.queries[q];
  const uint32_t flt = p.q_filter ? p.q_filter[q] : 0u;
  uint32_t *pct = reinterpret_cast<uint32_t *>(av_lds);
  unsigned long long *vals = XLDS ? av_lds + p.pct_words / 2 : p.values + (size_t)q * p.value_cells;
  uint32_t *scratch = p.scratch + (size_t)q * p.scratch_words;
  uint32_t *bits = XLDS ? reinterpret_cast<uint32_t *>(vals + p.value_cells) : scratch;
  if (XLDS) {
    uint32_t *w = reinterpret_cast<uint32_t *>(vals);
    for (uint32_t i = tid; i < 2 * p.value_cells + p.card_words; i += kAggThreads) w[i] = 0u;
  }
  __syncthreads();

  if (p.walk1) {
    agg_walk<true>(p, qr, flt, wave, lane, [&](const bool ok, const uint32_t seg, const uint32_t doc) {
      for (uint32_t v = 0; v < p.n_nodes; v++) {
        const AggNodeDev &n = p.nodes[v];
        if (n.kind == kAggCardinality) {
          if (!ok) continue;
          const uint32_t *ranks = p.rank_cols[(size_t)n.col * p.n_segs + seg];
          const ColumnDev col = p.cols[(size_t)n.col * p.n_segs + seg];
          uint32_t a, e;
          column_range(col, doc, a, e);
          const bool miss = e == a;
          const uint32_t nr = miss ? (n.has_missing && n.miss_rank < n.n_ranks ? 1u : 0u) : e - a;
          if (nr == 0) continue;
          auto into = [&](const uint32_t row) {
            uint32_t *rw = bits + n.bm_off + (size_t)row * n.wpr;
            for (uint32_t i = 0; i < nr; i++) {
              const uint32_t r = miss ? n.miss_rank : ranks[a + i];
              if (r >= n.n_ranks) continue;  // (registration refuses such a column)
              const uint32_t bit = 1u << (r & 31);
              // a stale read only repeats an atomic that changes nothing
              if (!(rw[r >> 5] & bit)) atomicOr(&rw[r >> 5], bit);
            }
          };
          if (n.parent < 0) into(0);
          else agg_buckets<EXT>(p, p.nodes[n.parent], seg, doc, into);
        } else if (n.kind == kAggPercentileRanks) {
          const uint32_t width = 1u + n.n_ranges;
          AggDocValues d{nullptr, 0u, 0u, false, 0.0};
          if (ok) d = agg_doc_values(p, n, seg, doc);
          if (n.parent < 0) {  // one row: a sum over the wave, then one atomic per counter
            const uint32_t tot = wave_sum(d.nv);
            if (tot == 0) continue;  // (wave-uniform)
            if (lane == 0) atomicAdd(&vals[n.off], (unsigned long long)tot);
            for (uint32_t t = 0; t < n.n_ranges; t++) {
              uint32_t c = 0;
              for (uint32_t i = 0; i < d.nv; i++) c += d.x(i) <= n.from[t] ? 1u : 0u;
              c = wave_sum(c);
              if (lane == 0 && c) atomicAdd(&vals[n.off + 1 + t], (unsigned long long)c);
            }
          } else if (d.nv) {
            agg_buckets<EXT>(p, p.nodes[n.parent], seg, doc, [&](const uint32_t row) {
              unsigned long long *cell = vals + n.off + (size_t)row * width;
              atomicAdd(&cell[0], (unsigned long long)d.nv);
              for (uint32_t t = 0; t < n.n_ranges; t++) {
                uint32_t c = 0;
                for (uint32_t i = 0; i < d.nv; i++) c += d.x(i) <= n.from[t] ? 1u : 0u;
                if (c) atomicAdd(&cell[1 + t], (unsigned long long)c);
              }
            });
          }
        }
      }
    });
    __syncthreads();
    // the popcount of every bitmap row: a thread per row while rows are short, else a wave per row
    for (uint32_t v = 0; v < p.n_nodes; v++) {
      const AggNodeDev &n = p.nodes[v];
      if (n.kind != kAggCardinality) continue;
      const uint32_t prow = n.parent < 0 ? 1u : p.nodes[n.parent].rows;
      const uint32_t *bm = bits + n.bm_off;
      if (n.wpr <= 8) {
        for (uint32_t row = tid; row < prow; row += kAggThreads) {
          uint32_t c = 0;
          for (uint32_t w = 0; w < n.wpr; w++) c += __popc(agg_read_back<!XLDS>(bm + (size_t)row * n.wpr + w));
          vals[n.off + row] = c;
        }
      } else {
        for (uint32_t row = wave; row < prow; row += kAggThreads / 64) {
          uint32_t c = 0;
          for (uint32_t w = lane; w < n.wpr; w += 64) c += __popc(agg_read_back<!XLDS>(bm + (size_t)row * n.wpr + w));
          c = wave_sum(c);
          if (lane == 0) vals[n.off + row] = c;
        }
      }
    }
  }

  for (uint32_t v = 0; v < p.n_nodes; v++) {
    const AggNodeDev &n = p.nodes[v];
    if (n.kind != kAggPercentiles) continue;
    const uint32_t *const *ranks_of = p.rank_cols + (size_t)n.col * p.n_segs;
    const uint32_t shift = n.shift, n_k = 2 * n.n_ranges;
    const uint32_t bins = ((n.n_ranks - 1u) >> shift) + 1u;  // <= 4096
    // every rank of an accepted doc: f(rank)
    auto each_rank = [&](auto &&f) {
      agg_walk<false>(p, qr, flt, wave, lane, [&](bool, const uint32_t seg, const uint32_t doc) {
        const ColumnDev col = p.cols[(size_t)n.col * p.n_segs + seg];
        uint32_t a, e;
        column_range(col, doc, a, e);
        if (e == a) {
          if (n.has_missing) f(n.miss_rank);
          return;
        }
        const uint32_t *ranks = ranks_of[seg];
        for (uint32_t i = a; i < e; i++) {
          const uint32_t r = ranks[i];
          const uint32_t rr = r + (r >= n.shift_from ? 1u : 0u);
          if (rr < n.n_ranks) f(rr);
        }
      });
    };
    __syncthreads();  // (the region is the previous node's)
    for (uint32_t i = tid; i < bins; i += kAggThreads) pct[i] = 0u;
    for (uint32_t i = tid; i < (1u << kAggCoarseBits) / 32; i += kAggThreads) sh_selmap[i] = 0u;
    __syncthreads();
    each_rank([&](const uint32_t r) { atomicAdd(&pct[r >> shift], 1u); });
    __syncthreads();
    // exclusive prefix sums in place: 16 consecutive bins per thread, a scan of the 256 partial sums
    {
      constexpr uint32_t kPer = (1u << kAggCoarseBits) / kAggThreads;
      const uint32_t b0 = tid * kPer;
      uint32_t sum = 0;
      for (uint32_t j = 0; j < kPer; j++) sum += b0 + j < bins ? pct[b0 + j] : 0u;
      const uint32_t ex = wave_excl_scan(sum, lane);
      if (lane == 63) sh_wtot[wave] = ex + sum;
      __syncthreads();
      uint32_t run = ex;
      for (uint32_t w = 0; w < wave; w++) run += sh_wtot[w];
      for (uint32_t j = 0; j < kPer; j++) {
        if (b0 + j >= bins) break;
        const uint32_t c = pct[b0 + j];
        pct[b0 + j] = run;
        run += c;
      }
      if (tid == kAggThreads - 1) sh_n = run;
      __syncthreads();
    }
    const uint32_t n_vals = sh_n;
    if (n_vals == 0) {  // (workgroup-uniform) QuantileState::percentile of nothing: the host returns 0.0
      for (uint32_t i = tid; i < 1u + n_k; i += kAggThreads) vals[n.off + i] = 0ull;
      continue;
    }
    if (tid < n_k) {
      // rank = (clamp(p, 0, 100) / 100) * (n - 1), low = floor, high = ceil: IEEE f64 (aggs/mod.rs:529-532)
      const double pc = fmin(fmax(n.from[tid >> 1], 0.0), 100.0);
      const double rank = fmax((pc / 100.0) * ((double)n_vals - 1.0), 0.0);
      const uint32_t k = (uint32_t)((tid & 1u) ? ceil(rank) : floor(rank));
      uint32_t lo = 0, hi = bins - 1u;  // the largest bin whose exclusive prefix is <= k holds element k
      while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (pct[mid] <= k) lo = mid;
        else hi = mid - 1u;
      }
      sh_kbin[tid] = lo;
      sh_kres[tid] = k - pct[lo];
    }
    __syncthreads();
    if (tid == 0) vals[n.off] = n_vals;
    if (shift == 0) {  // a bin is a rank
      if (tid < n_k) vals[n.off + 1 + tid] = (unsigned long long)__double_as_longlong(agg_rank_value(n, sh_kbin[tid]));
      continue;
    }
    if (tid == 0) {  // the distinct selected bins
      uint32_t ns = 0;
      for (uint32_t t = 0; t < n_k; t++) {
        uint32_t s = 0;
        while (s < ns && sh_selbin[s] != sh_kbin[t]) s++;
        if (s == ns) {
          sh_selbin[ns++] = sh_kbin[t];
          sh_selmap[sh_kbin[t] >> 5] |= 1u << (sh_kbin[t] & 31);
        }
        sh_ksel[t] = s;
      }
      sh_nsel = ns;
    }
    __syncthreads();
    const uint32_t n_sel = sh_nsel, mask = (1u << shift) - 1u;
    uint32_t *fine = n.fine_lds ? pct : scratch + n.fine_off;
    if (n.fine_lds) {  // (the prefix sums are used up; a global table was zeroed by the memset)
      for (uint32_t i = tid; i < (n_sel << shift); i += kAggThreads) pct[i] = 0u;
      __syncthreads();
    }
    each_rank([&](const uint32_t r) {
      const uint32_t b = r >> shift;
      if (!((sh_selmap[b >> 5] >> (b & 31)) & 1u)) return;
      uint32_t s = 0;
      while (s + 1 < n_sel && sh_selbin[s] != b) s++;
      if (n.fine_lds) atomicAdd(&pct[(s << shift) | (r & mask)], 1u);
      else atomicAdd(&fine[((size_t)s << shift) | (r & mask)], 1u);
    });
    __syncthreads();
    for (uint32_t t = wave; t < n_k; t += kAggThreads / 64) {  // a wave per order statistic
      const uint32_t *row = fine + ((size_t)sh_ksel[t] << shift);
      const uint32_t res = sh_kres[t];
      uint32_t run = 0, low = mask;
      for (uint32_t c0 = 0; c0 <= mask; c0 += 64) {
        const uint32_t idx = c0 + lane;
        uint32_t c = 0;
        if (idx <= mask) c = n.fine_lds ? row[idx] : agg_read_back<true>(row + idx);
        const uint32_t incl = run + wave_excl_scan(c, lane) + c;
        const uint64_t hit = __ballot(incl > res);
        if (hit) {
          low = c0 + (uint32_t)__builtin_ctzll(hit);
          break;
        }
        run = rl(incl, 63);
      }
      if (lane == 0)
        vals[n.off + 1 + t] =
            (unsigned long long)__double_as_longlong(agg_rank_value(n, (sh_kbin[t] << shift) | low));
    }
  }
  if (XLDS) {
    __syncthreads();
    unsigned long long *o = p.values + (size_t)q * p.value_cells;
    for (uint32_t i = tid; i < p.value_cells; i += kAggThreads) o[i] = vals[i];
  }
}

}  // namespace slg
