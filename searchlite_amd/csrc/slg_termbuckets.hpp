// slg_termbuckets.hpp — significant_terms and rare_terms (slg_batch_prepare_term_buckets; SignificantTermsCollector,
// RareTermsCollector, compute_background_counts, merge_significant_bucket_lists and finalize, query/aggs/mod.rs:131-359,
// :2110-2181, :2395-2424, :2515-2595).  Both kinds select at most `size` rows of a keyword's dense count table, so
// the tables stay where they are filled and `size` rows leave the device.  Four kernels:
//
// bg_count_kernel (at prepare, once per distinct (field, background filter) pair and segment): a lane per doc of the
//   segment; a doc whose tombstone or filter-reject bit is set is skipped; every other doc adds one to the segment's
//   bg_total and one to bg[seg][ord] per DISTINCT ordinal (the loop over the doc's earlier values, as agg_buckets).
//   LDS: 4 * n_ords <= kAggLdsBytes: a workgroup counts into LDS and flushes once with global atomics; else global
//   atomics directly.  Integer adds: both homes give the same table, whatever the order.
// term_bucket_count_kernel (behind agg_kernel): one workgroup per query over the candidates, as agg_walk walks them.
//   Per node a collected doc adds one to fg[ord] per distinct ordinal and one to the node's doc_count when it has a
//   value.  A significant node tests and sets the presence bit of (segment, ord) with an atomic OR; the ONE lane whose
//   OR returned the bit clear adds bg[seg][ord] to bgsum[ord]: the sum of the background counts of the segments in
//   whose foreground the key occurs, the reference's merge.  Which lane adds depends on arrival, what is added does
//   not.  The bit is read first, past the L1 (it is only ever set: a stale clear read repeats an atomic that decides
//   the same).  fg takes the two homes of agg_kernel's tables: LDS when 4 B per ordinal of every node fit
//   kAggLdsBytes, written out once, else the query's slice of the batch's table; the presence words and bgsum are
//   touched once per (segment, key) and live in device memory, zeroed on the batch's stream.
// term_bucket_select_kernel: one workgroup per (query, node) over the dense fg row.  A qualifying row is packed into
//   (significant ? ~fg : fg) << 32 | rank(ord); the `size` smallest packed keys are the reference's truncation under
//   (count desc | asc, key asc).  The selection is composite_select_kernel's per-wave threshold set (CpSet,
//   slg_cpset.hpp) with table rows as input.  A significant node then scores each kept row with three IEEE f64 divisions and orders the rows by
//   (score desc, count desc, rank asc): every thread counts the rows in front of its own (at most 1024 x 1024
//   compares of LDS words; the keys are distinct, so the counts are a permutation).  With children the kept ordinals
//   are ranked by ordinal the same way, with the row each maps to.
// term_bucket_collect_kernel (per node with children): composite_collect_kernel with the ordinal list in the place of
//   the key list: a collected doc's distinct ordinals are binary-searched, a hit in row r adds one to count cell r and
//   runs every child through agg_collect with cell = child.off + r * child.rows.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_aggs.hpp"
#include "slg_cpset.hpp"
#include "slg_wave.hpp"

namespace slg {

constexpr uint32_t kTbThreads = kAggThreads;
constexpr uint32_t kTbMaxNodes = 4;     // SLG_MAX_TERM_BUCKET_NODES
constexpr uint32_t kTbMaxSize = 1024;   // SLG_MAX_TERM_BUCKET_SIZE (the per-wave set holds kCpMaxSize + 1 keys)
constexpr uint32_t kTbBgBlocks = 1024;  // workgroups of bg_count_kernel at the most (a grid-stride loop beyond)
enum : uint32_t { kTbSignificant = 0, kTbRare = 1 };

struct TermBucketNodeDev {
  uint32_t kind, size;
  uint32_t n_ords, cap;            // cap: entries of one wave's set in the select (cp_cap(size))
  unsigned long long bound;        // significant: min_doc_count; rare: max_doc_count
  const uint32_t *ord_rank;        // the rank of every ordinal in key byte order, or null (the ordinal is the rank)
  const uint32_t *rank_ord;        // its inverse, or null
  const uint32_t *bg;              // significant: [n_segs][n_ords + 1], bg_total of the segment in the last cell
  uint32_t fg_off;                 // first cell of the node in a query's fg / bgsum row
  uint32_t bits_off, wpr;          // significant: first presence word of the node, words per segment
  uint32_t row_off;                // first row of the node in a query's output rows
  uint32_t n_children, pad;
};

struct TermBucketParams {
  AggParams a;  // the candidates.  The collect: nodes / cols / n_nodes = the children of ONE node, count_cells /
                // stats_cells = the cells of that node's tables, counts / stats = its first cell in query 0's row
  const TermBucketNodeDev *tb;  // [n_tb]
  const ColumnDev *tb_cols;     // [n_tb * n_segs]
  uint32_t n_tb, node;          // node: the collect's
  uint32_t fg_cells, bits_words, rows;  // of one query: cells of fg / bgsum, presence words, output rows
  uint32_t cnt_stride, st_stride;       // the collect: cells of one query's row of the batch's term-bucket tables
  uint32_t *fg;                 // [nq * fg_cells]
  unsigned long long *bgsum;    // [nq * fg_cells]
  uint32_t *bits;               // [nq * bits_words]
  unsigned long long *doc_counts, *bg_counts, *score_bits;  // [nq * rows]
  unsigned long long *node_dc, *node_bg;                    // [nq * n_tb]
  uint32_t *ords;               // [nq * rows]
  uint32_t *n_buckets;          // [nq * n_tb]
  uint32_t *sorted_ords, *row_of;  // [nq * rows] the kept ordinals in ordinal order, the row of each
  uint32_t *err;                // the word behind n_buckets: ...
  const uint32_t *flag;         // ... the index's error word as the batch's last kernel left it
};

struct BgCountParams {
  ColumnDev col;
  const uint32_t *deleted, *reject;  // bitmaps or null
  uint32_t n_docs, n_ords;
  uint32_t *bg;  // [n_ords + 1] of this segment, zeroed
};

// f(o) once per DISTINCT ordinal of the doc's values [a, e) (an ordinal beyond the dictionary: registration refuses
// such a column)
template <typename F>
__device__ __forceinline__ void tb_distinct_ords(const uint32_t *v, const uint32_t a, const uint32_t e,
                                                 const uint32_t n_ords, F &&f) {
  for (uint32_t i = a; i < e; i++) {
    const uint32_t o = v[i];
    if (o >= n_ords) continue;
    bool dup = false;
    for (uint32_t j = a; j < i; j++) dup = dup || v[j] == o;
    if (dup) continue;
    f(o);
  }
}

template <bool LDS>
static __global__ void __launch_bounds__(kTbThreads) bg_count_kernel(BgCountParams p) {
  extern __shared__ uint32_t bg_lds[];  // (LDS) [n_ords]
  __shared__ uint32_t sh_total;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  if (tid == 0) sh_total = 0;
  if (LDS)
    for (uint32_t i = tid; i < p.n_ords; i += kTbThreads) bg_lds[i] = 0u;
  __syncthreads();
  uint32_t *tab = LDS ? bg_lds : p.bg;
  const uint32_t *v = p.col.ords();
  uint32_t total = 0;
  for (uint32_t d0 = blockIdx.x * kTbThreads; d0 < p.n_docs; d0 += gridDim.x * kTbThreads) {
    const uint32_t doc = d0 + tid;
    if (doc >= p.n_docs) continue;
    if (p.deleted && ((p.deleted[doc >> 5] >> (doc & 31)) & 1u)) continue;
    if (p.reject && ((p.reject[doc >> 5] >> (doc & 31)) & 1u)) continue;
    total++;
    if (!p.col.vals) continue;
    uint32_t a, e;
    column_range(p.col, doc, a, e);
    tb_distinct_ords(v, a, e, p.n_ords, [&](const uint32_t o) { atomicAdd(&tab[o], 1u); });
  }
  total = wave_sum(total);
  if (lane == 0 && total) atomicAdd(&sh_total, total);
  __syncthreads();
  if (tid == 0 && sh_total) atomicAdd(&p.bg[p.n_ords], sh_total);
  if (LDS)
    for (uint32_t i = tid; i < p.n_ords; i += kTbThreads)
      if (bg_lds[i]) atomicAdd(&p.bg[i], bg_lds[i]);
}

template <bool LDS>
static __global__ void __launch_bounds__(kTbThreads) term_bucket_count_kernel(TermBucketParams p) {
  extern __shared__ uint32_t tc_lds[];  // (LDS) fg [fg_cells]
  __shared__ unsigned long long sh_dc[kTbMaxNodes];
  __shared__ uint32_t sh_matched;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t q = blockIdx.x;
  if (q >= p.a.nq) return;
  if (tid == 0) sh_matched = 0;
  const QueryRef qr = p.a.queries[q];
  const uint32_t flt = p.a.q_filter ? p.a.q_filter[q] : 0u;
  unsigned long long *bgsum = p.bgsum + (size_t)q * p.fg_cells;
  uint32_t *fg = LDS ? tc_lds : p.fg + (size_t)q * p.fg_cells;
  uint32_t *bits = p.bits + (size_t)q * p.bits_words;
  if (tid < kTbMaxNodes) sh_dc[tid] = 0ull;
  if (LDS)
    for (uint32_t i = tid; i < p.fg_cells; i += kTbThreads) tc_lds[i] = 0u;
  __syncthreads();

  uint32_t dc[kTbMaxNodes] = {0u, 0u, 0u, 0u};
  uint32_t nv = 0;
  agg_walk<false>(p.a, qr, flt, wave, lane, [&](bool, const uint32_t seg, const uint32_t doc) {
    nv++;
#pragma unroll
    for (uint32_t n = 0; n < kTbMaxNodes; n++) {
      if (n >= p.n_tb) continue;
      const TermBucketNodeDev &t = p.tb[n];
      const ColumnDev col = p.tb_cols[(size_t)n * p.a.n_segs + seg];
      uint32_t a, e;
      column_range(col, doc, a, e);
      if (e == a) continue;
      dc[n]++;
      tb_distinct_ords(col.ords(), a, e, t.n_ords, [&](const uint32_t o) {
        atomicAdd(&fg[t.fg_off + o], 1u);
        if (t.kind != kTbSignificant) return;
        uint32_t *w = bits + t.bits_off + (size_t)seg * t.wpr + (o >> 5);
        const uint32_t bit = 1u << (o & 31);
        // the lane that flips the bit adds the segment's background count of the key, once per (segment, key)
        if (!(agg_read_back<true>(w) & bit) && !(atomicOr(w, bit) & bit))
          atomicAdd(&bgsum[t.fg_off + o], (unsigned long long)t.bg[(size_t)seg * (t.n_ords + 1u) + o]);
      });
    }
  });
#pragma unroll
  for (uint32_t n = 0; n < kTbMaxNodes; n++) {
    const uint32_t s = wave_sum(dc[n]);
    if (lane == 0 && s) atomicAdd(&sh_dc[n], (unsigned long long)s);
  }
  nv = wave_sum(nv);
  if (lane == 0 && nv) atomicAdd(&sh_matched, nv);
  __syncthreads();
  if (tid == 0 && p.a.out_matched) p.a.out_matched[q] = sh_matched;
  if (tid < p.n_tb) p.node_dc[(size_t)q * p.n_tb + tid] = sh_dc[tid];
  if (LDS) {
    uint32_t *of = p.fg + (size_t)q * p.fg_cells;
    for (uint32_t i = tid; i < p.fg_cells; i += kTbThreads) of[i] = fg[i];
  }
}

// (a, b) < (c, d)
__device__ __forceinline__ bool tb_less(const unsigned long long a, const unsigned long long b,
                                        const unsigned long long c, const unsigned long long d) {
  return a < c || (a == c && b < d);
}

static __global__ void __launch_bounds__(kTbThreads) term_bucket_select_kernel(TermBucketParams p) {
  extern __shared__ unsigned long long ts_lds[];  // the four waves' sets; then wave 1's: ~score bits, wave 2's: ordinals
  __shared__ uint32_t sh_n[kCpWaves];
  __shared__ unsigned long long sh_bg;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t q = blockIdx.x, n = blockIdx.y;
  if (q >= p.a.nq || n >= p.n_tb) return;
  const TermBucketNodeDev t = p.tb[n];
  const bool sig = t.kind == kTbSignificant;
  if (q == 0 && n == 0 && tid == 0) *p.err = *p.flag;
  const uint32_t *fg = p.fg + (size_t)q * p.fg_cells + t.fg_off;
  const unsigned long long *bgsum = p.bgsum + (size_t)q * p.fg_cells + t.fg_off;
  CpSet set{ts_lds + (size_t)wave * t.cap, t.cap, t.size, 0u, kCpEmpty};
  set.clear(lane);
  if (tid == 0) {  // the node's bg_count: every segment's bg_total, a segment without a match too
    unsigned long long s = 0;
    if (sig)
      for (uint32_t seg = 0; seg < p.a.n_segs; seg++) s += t.bg[(size_t)seg * (t.n_ords + 1u) + t.n_ords];
    sh_bg = s;
  }
  const unsigned long long lo_bound = t.bound > 1ull ? t.bound : 1ull;
  for (uint32_t o0 = wave * 64u; o0 < t.n_ords; o0 += kTbThreads) {  // (wave-uniform bounds: offer is wave-wide)
    const uint32_t o = o0 + lane;
    const uint32_t c = o < t.n_ords ? fg[o] : 0u;
    const bool has = sig ? (unsigned long long)c >= lo_bound : (c >= 1u && (unsigned long long)c <= t.bound);
    const uint32_t rank = has ? (t.ord_rank ? t.ord_rank[o] : o) : 0u;
    set.offer(has, ((unsigned long long)(sig ? ~c : c) << 32) | rank, lane);
  }
  if (wave != 0u) {
    set.sort(lane);
    if (lane == 0) sh_n[wave] = set.count < t.size + 1u ? set.count : t.size + 1u;
  }
  __syncthreads();
  if (wave == 0u) {
    for (uint32_t w = 1; w < kCpWaves; w++) {
      const unsigned long long *L = ts_lds + (size_t)w * t.cap;
      const uint32_t m = sh_n[w];
      for (uint32_t i0 = 0; i0 < m; i0 += 64) {
        const bool has = i0 + lane < m;
        set.offer(has, has ? L[i0 + lane] : kCpEmpty, lane);
      }
    }
    set.sort(lane);
    if (lane == 0) sh_n[0] = set.count < t.size ? set.count : t.size;
  }
  __syncthreads();
  // the kept rows: ts_lds[0 .. nb) ascending, the reference's truncated list in (count, key) order
  const uint32_t nb = sh_n[0];
  const unsigned long long *K = ts_lds;
  unsigned long long *S = ts_lds + t.cap;       // ~score bits (cap >= 2 * (size + 1) entries each)
  unsigned long long *O = ts_lds + 2u * t.cap;  // the ordinals
  const unsigned long long dc = p.node_dc[(size_t)q * p.n_tb + n], bgt = sh_bg;
  for (uint32_t i = tid; i < nb; i += kTbThreads) {
    const unsigned long long key = K[i];
    const uint32_t rank = (uint32_t)key;
    const uint32_t o = t.rank_ord ? t.rank_ord[rank] : rank;
    unsigned long long sb = 0ull;
    if (sig) {
      const uint32_t c = ~(uint32_t)(key >> 32);
      const unsigned long long b = bgsum[o];
      // (b.doc_count / doc_count) / (b.bg_count / bg_count): three IEEE f64 divisions (no fast-math); 0.0 when a
      // denominator's count is zero.  A score is finite and not negative: its bits order as it does
      double score = 0.0;
      if (dc > 0ull && bgt > 0ull && b > 0ull) score = ((double)c / (double)dc) / ((double)b / (double)bgt);
      sb = (unsigned long long)__double_as_longlong(score);
    }
    S[i] = ~sb;
    O[i] = o;
  }
  __syncthreads();
  const size_t row0 = (size_t)q * p.rows + t.row_off;
  for (uint32_t i = tid; i < t.size; i += kTbThreads) {
    if (i >= nb) {  // rows past n_buckets are zero
      p.ords[row0 + i] = 0u;
      p.doc_counts[row0 + i] = p.bg_counts[row0 + i] = p.score_bits[row0 + i] = 0ull;
      continue;
    }
    const unsigned long long key = K[i], s = S[i], o = O[i];
    uint32_t pos = i, opos = 0;
    if (sig) {  // rows in front under (score desc, count desc, rank asc); a rare node keeps the selection order
      pos = 0;
      for (uint32_t j = 0; j < nb; j++) pos += tb_less(S[j], K[j], s, key) ? 1u : 0u;
    }
    if (t.n_children) {
      for (uint32_t j = 0; j < nb; j++) opos += O[j] < o ? 1u : 0u;
      p.sorted_ords[row0 + opos] = (uint32_t)o;
      p.row_of[row0 + opos] = pos;
    }
    const uint32_t c = sig ? ~(uint32_t)(key >> 32) : (uint32_t)(key >> 32);
    p.ords[row0 + pos] = (uint32_t)o;
    p.doc_counts[row0 + pos] = c;
    p.bg_counts[row0 + pos] = sig ? bgsum[o] : 0ull;
    p.score_bits[row0 + pos] = sig ? ~s : 0ull;
  }
  if (tid == 0) {
    p.n_buckets[(size_t)q * p.n_tb + n] = nb;
    p.node_bg[(size_t)q * p.n_tb + n] = bgt;  // (a rare node's doc_count is dropped by the fetch)
  }
}

template <bool LDS, bool EXT>
static __global__ void __launch_bounds__(kTbThreads) term_bucket_collect_kernel(TermBucketParams p) {
  extern __shared__ unsigned long long tl_lds[];  // (LDS) the stats cells, the count cells; then the ordinals, their rows
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t q = blockIdx.x;
  if (q >= p.a.nq) return;
  const TermBucketNodeDev &t = p.tb[p.node];
  const QueryRef qr = p.a.queries[q];
  const uint32_t flt = p.a.q_filter ? p.a.q_filter[q] : 0u;
  const uint32_t nb = p.n_buckets[(size_t)q * p.n_tb + p.node];
  const uint32_t tab_words = LDS ? 8u * p.a.stats_cells + p.a.count_cells : 0u;
  AggStatDev *st = LDS ? reinterpret_cast<AggStatDev *>(tl_lds) : p.a.stats + (size_t)q * p.st_stride;
  uint32_t *cnt = LDS ? reinterpret_cast<uint32_t *>(tl_lds + 4 * (size_t)p.a.stats_cells)
                      : p.a.counts + (size_t)q * p.cnt_stride;
  uint32_t *so = reinterpret_cast<uint32_t *>(tl_lds) + tab_words;
  uint32_t *ro = so + t.size;
  const size_t row0 = (size_t)q * p.rows + t.row_off;
  for (uint32_t i = tid; i < nb; i += kTbThreads) {
    so[i] = p.sorted_ords[row0 + i];
    ro[i] = p.row_of[row0 + i];
  }
  if (LDS) {
    uint32_t *w = reinterpret_cast<uint32_t *>(tl_lds);
    for (uint32_t i = tid; i < tab_words; i += kTbThreads) w[i] = 0u;  // every cell starts as zero words
  }
  __syncthreads();

  const uint32_t n_ords = t.n_ords;
  if (nb != 0u)
    agg_walk<false>(p.a, qr, flt, wave, lane, [&](bool, const uint32_t seg, const uint32_t doc) {
      const ColumnDev col = p.tb_cols[(size_t)p.node * p.a.n_segs + seg];
      uint32_t a, e;
      column_range(col, doc, a, e);
      tb_distinct_ords(col.ords(), a, e, n_ords, [&](const uint32_t o) {
        uint32_t lo = 0, hi = nb;  // the first kept ordinal >= o
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (so[mid] < o) lo = mid + 1u;
          else hi = mid;
        }
        if (lo == nb || so[lo] != o) return;
        const uint32_t r = ro[lo];
        atomicAdd(&cnt[r], 1u);
        for (uint32_t c = 0; c < p.a.n_nodes; c++) {
          const AggNodeDev &ch = p.a.nodes[c];
          agg_collect<EXT>(p.a, ch, seg, doc, ch.off + r * ch.rows, cnt, st, [](uint32_t) {});
        }
      });
    });
  if (LDS) {
    __syncthreads();
    uint32_t *oc = p.a.counts + (size_t)q * p.cnt_stride;
    for (uint32_t i = tid; i < p.a.count_cells; i += kTbThreads) oc[i] = cnt[i];
    unsigned long long *os = reinterpret_cast<unsigned long long *>(p.a.stats + (size_t)q * p.st_stride);
    for (uint32_t i = tid; i < 4 * p.a.stats_cells; i += kTbThreads) os[i] = tl_lds[i];
  }
}

}  // namespace slg
