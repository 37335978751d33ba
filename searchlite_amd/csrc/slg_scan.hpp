// slg_scan.hpp — the candidate source of a scan batch (slg_batch_prepare_scan): match_all, constant_score and
// rank_feature at the root, the reference's scan_segment (api/reader.rs:3131-3236) as one kernel in the place of
// the partition and scoring kernels.  The semantics in full: include/searchlite_gpu.h.  In short, per doc of a
// segment: it matches when no reject bitmap has its bit — the node's own filter, the batch's root filter (both
// hold deleted | ~filter), or the segment's `deleted` when neither is set; match_all scores 1.0, constant_score
// its score, rank_feature (float)modifier(first value of the column as f64, or (double)missing) * boost, and a
// non-finite modified value or product drops the doc.  f64 arithmetic, one operation at a time (the unit is built
// with -ffp-contract=off and without fast-math).
//
// Output: the format every batch's selects and aggregation kernels read.  A slice's survivors are written as
// {ordered key of the f32 score, doc} in ascending doc order to the front of its region (slice_cbeg[s]; `cap`
// entries), slice_ccnt[s] is the stored count, and the slice's TRUE count is added to the query's scored and
// matched counters with one atomic each.  In the truncated form (cap < the slice's docs: every score of the query
// is equal and nothing but the top k reads the region) stores stop at cap while counting goes on.
//
// Shape: the clause filters' — one wave per slice, four per workgroup.  A step covers 2048 docs: lane l reads word
// l of the step from each bitmap (one 256-byte row per bitmap), ORs them into its pass word and masks the bits at
// and beyond the slice's end; words beyond the slice's last are never read.  A step whose pass words are all zero
// costs nothing more; in the truncated form a step behind a full region is a popcount.  Otherwise the step is 32
// rounds of 64 docs: the round's two pass words come from the lanes that hold them (readlane; a round without a
// bit is skipped), every lane tests its doc's bit, rank_feature lanes gather offsets[doc], offsets[doc + 1] (none
// when the column is stored without offsets) and values[first] and turn a drop into a cleared bit, and the
// survivors are ranked with ballot + mbcnt and stored lane-contiguously.  The slice's record, the query's record,
// the bitmap and column addresses are wave-uniform and read through the constant address space (scalar loads).
//
// FULL = false compiles the kernel without ln / log1p (the device library's f64 forms are the register-heavy part):
// the host launches it for batches without a LOG or LOG1P query.
#pragma once

#include "slg_wave.hpp"

namespace slg {

constexpr int kScanThreads = 256;  // four waves = four slices per workgroup

struct ScanParams {
  const SegDev *segs;
  const ScanQuery *queries;             // [nq]
  const ScanSlice *slices;              // [n_slices]
  const ColumnDev *cols;                // [fields of the batch][n_segs]
  const uint32_t *q_filter;             // [nq] the root filters: 0 = none, f + 1; or null
  const uint32_t *const *reject_table;  // [n_filters * n_segs] reject bitmaps of the batch's state
  uint2 *cand;
  const uint64_t *slice_cbeg;
  uint32_t *slice_ccnt;
  uint32_t *q_scored;                   // [nq] zeroed in front of the kernel
  unsigned long long *q_matched;        // [nq] the same
  uint32_t n_slices, n_segs;
};

// apply_rank_modifier (api/reader.rs:183-215), its branch conditions as they stand there
template <bool FULL>
__device__ __forceinline__ double scan_modifier(double x, uint32_t mod) {
  if (mod == kScanModSqrt) return x < 0.0 ? 0.0 : sqrt(x);
  if (mod == kScanModReciprocal) return x == 0.0 ? 0.0 : 1.0 / x;
  if constexpr (FULL) {
    if (mod == kScanModLog) return x <= 0.0 ? 0.0 : log(x);
    if (mod == kScanModLog1p) return x <= -1.0 ? 0.0 : log1p(x);
  }
  return x;
}

template <bool FULL>
static __global__ void __launch_bounds__(kScanThreads) scan_kernel(ScanParams p) {
  typedef const __attribute__((address_space(1))) uint32_t *gu32_t;
  typedef const __attribute__((address_space(1))) double *gf64_t;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = rfl(blockIdx.x * (kScanThreads / 64) + (threadIdx.x >> 6));
  if (s >= p.n_slices) return;
  const ScanSlice sl = load_const(p.slices + s);
  const uint32_t q = rfl(sl.q), seg = rfl(sl.seg), first = rfl(sl.first_doc), n_docs = rfl(sl.n_docs), cap = rfl(sl.cap);
  const ScanQuery sq = load_const(p.queries + q);
  const uint32_t kind = rfl(sq.kind), mod = rfl(sq.modifier);
  const uint32_t node = rfl(sq.filter), root = p.q_filter ? rfl(load_const(p.q_filter + q)) : 0u;
  // the reject bitmaps of the slice's segment (0: none).  A filter's bitmap holds deleted | ~filter
  uint64_t bm_node = 0ull, bm_root = 0ull, bm_del = 0ull;
  if (node) bm_node = uniform64((uint64_t)(uintptr_t)load_const(p.reject_table + ((size_t)(node - 1u) * p.n_segs + seg)));
  if (root) bm_root = uniform64((uint64_t)(uintptr_t)load_const(p.reject_table + ((size_t)(root - 1u) * p.n_segs + seg)));
  if (!node && !root) bm_del = uniform64((uint64_t)(uintptr_t)load_const(&p.segs[seg].deleted));
  uint64_t offs = 0ull, vals = 0ull;
  if (kind == kScanRankFeature) {
    const ColumnDev col = load_const(p.cols + ((size_t)rfl(sq.col) * p.n_segs + seg));
    offs = uniform64((uint64_t)(uintptr_t)col.offs);
    vals = uniform64((uint64_t)(uintptr_t)col.vals);
  }
  const double missing = (double)sq.missing;
  const uint32_t const_key = ordered_score(sq.score);
  uint2 *const reg = p.cand + uniform64(load_const(p.slice_cbeg + s));
  const uint32_t word0 = first >> 5;             // (first is a multiple of 2048)
  const uint32_t n_words = (n_docs + 31u) >> 5;  // words of the slice; its last one may be partial
  uint32_t stored = 0u, total = 0u;              // wave-uniform
  uint32_t lane_count = 0u;                      // per lane: docs counted behind a full region
  for (uint32_t wbase = 0; wbase < n_words; wbase += 64u) {
    const uint32_t wi = wbase + lane;
    uint32_t pass = 0u;
    if (wi < n_words) {
      uint32_t rej = 0u;
      if (bm_del) rej |= ((gu32_t)(uintptr_t)bm_del)[word0 + wi];
      if (bm_node) rej |= ((gu32_t)(uintptr_t)bm_node)[word0 + wi];
      if (bm_root) rej |= ((gu32_t)(uintptr_t)bm_root)[word0 + wi];
      pass = ~rej;
      const uint32_t left = n_docs - wi * 32u;  // docs of the slice from this word on: >= 1
      if (left < 32u) pass &= (1u << left) - 1u;
    }
    if (kind != kScanRankFeature && stored >= cap) {  // (truncated form, region full: nothing more is stored)
      lane_count += (uint32_t)__popc(pass);
      continue;
    }
    if (__ballot(pass != 0u) == 0ull) continue;
    for (uint32_t j = 0; j < 32u; j++) {
      const uint32_t w_lo = rl(pass, 2u * j), w_hi = rl(pass, 2u * j + 1u);
      if ((w_lo | w_hi) == 0u) continue;
      const uint32_t doc = first + (wbase + 2u * j) * 32u + lane;
      bool on = (((lane < 32u ? w_lo : w_hi) >> (lane & 31u)) & 1u) != 0u;
      uint32_t key = const_key;
      if (kind == kScanRankFeature) {
        uint32_t a = doc, e = doc + 1u;
        if (offs != 0ull && on) {
          a = ((gu32_t)(uintptr_t)offs)[doc];
          e = ((gu32_t)(uintptr_t)offs)[doc + 1u];
        }
        double raw = missing;
        if (on && a < e) raw = ((gf64_t)(uintptr_t)vals)[a];
        const double m = scan_modifier<FULL>(raw, mod);
        const float sc = (float)m * sq.boost;
        on = on && isfinite(m) && isfinite(sc);
        key = ordered_score(sc);
      }
      const uint64_t mask = __ballot(on);
      const uint32_t n = (uint32_t)__popcll(mask);
      const uint32_t at = stored + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
      if (on && at < cap) reg[at] = make_uint2(key, doc);
      total += n;
      stored = stored + n < cap ? stored + n : cap;
    }
  }
  total += wave_sum(lane_count);
  if (lane == 0u) {
    p.slice_ccnt[s] = stored;
    if (total) {
      atomicAdd(p.q_scored + q, total);
      atomicAdd(p.q_matched + q, (unsigned long long)total);
    }
  }
}

}  // namespace slg
