// slg_rescore.hpp — query rescore (SearchRequest::rescore, api/types.rs:523-545): a second BM25 query
// over the first w rows of each query, combined with the first-pass score and put back in order.
//
// Arithmetic restated: api/reader.rs:3238-3398 (rescore_hits: a row the rescore query does not match
// keeps its score, :3319-3321; a matched row's term scores are summed per leaf and the leaves combined
// by the query's score plan; hits[..window] alone is sorted again, :3393-3396) and :3623-3629
// (combine_rescore_scores).  The reference adds a row's term scores while walking a HashMap
// (:3290-3300), so its own order of additions is not defined; here it is fixed, as in the first pass:
// the terms of a leaf in query-term order, the leaves in leaf order.  The semantics in full:
// include/searchlite_gpu.h (slg_batch_prepare_rescore).
//
// The device index already holds what a term score needs: SegDev::docs / imps are doc-sorted lists
// with the BM25 impact of every posting at weight 1, so term_freq_for_doc + score_tf of one
// (row, term) is one search in docs[off .. off + df) and one imps[p] * weight.
//
// Shape: one workgroup of 256 threads per query, as the rerank kernels.  A lane owns up to four rows
// (row = thread + 256 * r) and runs their binary searches side by side, so four independent loads are
// in flight per lane and step: ceil(log2 df) dependent 4-byte loads narrow a list to one posting, one
// more compares it, one reads the impact.  A search stays inside [off, off + df): the sentinels behind
// a list and the null run are never probed.  No tombstone or filter test: first-pass rows are live.
// Wave 0 then emits the window in order through WaveTopK (top w of w candidates is the sort).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_wave.hpp"

namespace slg {

struct RescoreParams {
  const SegDev *segs;
  uint32_t n_segs;
  const RescoreQuery *queries;  // [nq]
  const RescoreTerm *terms;     // (slg_desc.hpp: [(term_begin + i) * n_segs + s])
  uint32_t *out_doc, *out_seg;  // the batch's rows [nq * k], rewritten in place
  float *out_score;
  const uint32_t *out_count;    // [nq]
  float *first_score, *rescore_score;  // [nq * k] parallel to the rows (slg_batch_fetch_rescore)
  uint32_t *rescored;
  uint32_t nq, k;
  uint32_t lds_rows;  // rows the LDS arrays hold: >= every query's window, even
};

constexpr int kRescoreThreads = 256;
constexpr int kRescoreRows = 4;  // rows per lane
static_assert(kRescoreThreads * kRescoreRows == (int)kRescoreMaxWindow, "a lane's rows cover the largest window");

inline size_t rescore_lds_bytes(uint32_t lds_rows, uint32_t max_table) {
  return (size_t)lds_rows * 12 + (size_t)max_table * sizeof(RescoreTerm);
}

// combine_rescore_scores (api/reader.rs:3623-3629); modes: SLG_RESCORE_* (searchlite_gpu.h)
__device__ __forceinline__ float rescore_combine(const uint32_t mode, const float o, const float r) {
  switch (mode) {
    case 1: return o * r;
    case 3: return fmaxf(o, r);
    case 4: return fminf(o, r);
    default: return o + r;  // total, sum
  }
}

template <int KREGS>
__global__ void __launch_bounds__(kRescoreThreads) rescore_kernel(RescoreParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int R = kRescoreRows;
  int32_t *s_tk = reinterpret_cast<int32_t *>(smem);  // [lds_rows] the window's keys: unsorted, then in order
  uint32_t *s_seg = reinterpret_cast<uint32_t *>(s_tk + p.lds_rows);
  uint32_t *s_doc = s_seg + p.lds_rows;
  RescoreTerm *s_terms = reinterpret_cast<RescoreTerm *>(s_doc + p.lds_rows);  // [n_terms * n_segs]
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t q = blockIdx.x, k = p.k, n_segs = p.n_segs;
  const RescoreQuery rq = p.queries[q];
  const uint32_t nt = rq.n_terms;
  uint32_t count = p.out_count[q];
  count = count < k ? count : k;
  uint32_t w = rq.window < count ? rq.window : count;
  w = w < p.lds_rows ? w : p.lds_rows;  // (the host sized the arrays for every window: a guard, not a path)
  if (nt == 0) w = 0;
  uint32_t *const odoc = p.out_doc + (size_t)q * k;
  uint32_t *const oseg = p.out_seg + (size_t)q * k;
  float *const oscore = p.out_score + (size_t)q * k;
  float *const ofirst = p.first_score + (size_t)q * k;
  float *const orsc = p.rescore_score + (size_t)q * k;
  uint32_t *const oflag = p.rescored + (size_t)q * k;
  // rows behind the window keep their place and score (rows past count hold zeros)
  for (uint32_t i = w + tid; i < k; i += kRescoreThreads) {
    ofirst[i] = oscore[i];
    orsc[i] = 0.0f;
    oflag[i] = 0u;
  }
  if (w == 0) return;

  {  // the query's term table, 8-byte words (RescoreTerm is three of them)
    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(p.terms + (size_t)rq.term_begin * n_segs);
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(s_terms);
    for (uint32_t i = tid; i < nt * n_segs * 3u; i += kRescoreThreads) dst[i] = src[i];
  }
  // this lane's rows
  typedef const __attribute__((address_space(1))) uint32_t *gdoc_t;
  typedef const __attribute__((address_space(1))) float *gimp_t;
  bool valid[R];
  uint32_t doc[R], seg[R], row_seg[R];
  float first[R];
  gdoc_t docs[R];
  gimp_t imps[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const uint32_t i = tid + kRescoreThreads * r;
    valid[r] = i < w;
    doc[r] = valid[r] ? odoc[i] : 0u;
    seg[r] = valid[r] ? oseg[i] : 0u;
    first[r] = valid[r] ? oscore[i] : 0.0f;
    row_seg[r] = seg[r];
    valid[r] = valid[r] && seg[r] < n_segs;  // (a row of no segment is looked up nowhere: it stays as it is)
    seg[r] = valid[r] ? seg[r] : 0u;
    const SegDev sd = p.segs[seg[r]];
    docs[r] = (gdoc_t)sd.docs;
    imps[r] = (gimp_t)sd.imps;
  }
  __syncthreads();

  // ---- the rescore score of every row: per-leaf sums in term order, leaves closed in leaf order ----
  const bool dismax = rq.plan != 0u;
  float acc[R], mx[R], leafv[R];
  uint32_t nhit[R];
  bool leafhit[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    acc[r] = dismax ? 0.0f : -0.0f;  // a DisMax sums from 0.0, a Sum from -0.0 (f32's Sum identity)
    mx[r] = -INFINITY;
    leafv[r] = 0.0f;
    nhit[r] = 0u;
    leafhit[r] = false;
  }
  for (uint32_t ti = 0; ti < nt; ti++) {
    uint64_t off[R];
    uint32_t n[R], pos[R];
    float wt[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const RescoreTerm t = s_terms[ti * n_segs + seg[r]];
      off[r] = t.off;
      n[r] = valid[r] ? t.df : 0u;
      wt[r] = t.weight;
      pos[r] = 0u;
    }
    // the last posting <= doc of each row's list (or posting 0): every probe lies in [off, off + df)
    bool more = false;
#pragma unroll
    for (int r = 0; r < R; r++) more = more || n[r] > 1u;
    while (more) {
      uint32_t v[R], half[R];
#pragma unroll
      for (int r = 0; r < R; r++) {
        half[r] = n[r] >> 1;
        v[r] = 0u;
        if (n[r] > 1u) v[r] = docs[r][off[r] + pos[r] + half[r]];
      }
      more = false;
#pragma unroll
      for (int r = 0; r < R; r++) {
        if (n[r] > 1u) {
          pos[r] = v[r] <= doc[r] ? pos[r] + half[r] : pos[r];
          n[r] -= half[r];
        }
        more = more || n[r] > 1u;
      }
    }
    uint32_t hit_doc[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      hit_doc[r] = kDocEnd;
      if (n[r] != 0u) hit_doc[r] = docs[r][off[r] + pos[r]];
    }
    float imp[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const bool found = n[r] != 0u && hit_doc[r] == doc[r];
      imp[r] = 0.0f;
      if (found) imp[r] = imps[r][off[r] + pos[r]];
      n[r] = found ? 1u : 0u;
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
      if (n[r]) {
        leafv[r] += imp[r] * wt[r];  // score_tf: base * weight, then the leaf's sum (no contraction)
        leafhit[r] = true;
      }
    }
    // (a term's leaf is the same in every segment: the close is uniform)
    const uint32_t leaf = s_terms[ti * n_segs].leaf;
    if (ti + 1 == nt || s_terms[(ti + 1) * n_segs].leaf != leaf) {
#pragma unroll
      for (int r = 0; r < R; r++) {
        if (leafhit[r]) {
          acc[r] += leafv[r];
          mx[r] = fmaxf(mx[r], leafv[r]);
          nhit[r]++;
        }
        leafv[r] = 0.0f;
        leafhit[r] = false;
      }
    }
  }
  float rsc[R], fresh[R];
  bool matched[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    matched[r] = valid[r] && nhit[r] >= rq.min_match;
    float rs = acc[r];
    if (dismax) {
      const float m = nhit[r] < rq.n_leaves ? fmaxf(mx[r], 0.0f) : mx[r];  // a leaf without a posting counts as 0.0
      rs = m + rq.tie * (acc[r] - m);
    }
    rsc[r] = matched[r] ? rs : 0.0f;
    fresh[r] = matched[r] ? rescore_combine(rq.mode, first[r], rs) : first[r];
    const uint32_t i = tid + kRescoreThreads * r;
    if (i < w) {
      s_tk[i] = total_key(fresh[r]);
      s_seg[i] = row_seg[r];
      s_doc[i] = doc[r];
    }
  }
  __syncthreads();

  // ---- wave 0: the window in order (top w of w), back into the rows and into LDS for the detail arrays ----
  if (tid < 64u) {
    WaveTopK<KREGS, true> top;
    top.init();
    for (uint32_t base = 0; base < w; base += 64) {
      const uint32_t i = base + lane;
      const bool have = i < w;
      const int32_t ctk = have ? s_tk[i] : kSentinelTk;
      const uint32_t cs = have ? s_seg[i] : 0xFFFFFFFFu, cd = have ? s_doc[i] : 0xFFFFFFFFu;
      top.offer(have, ctk, cs, cd, w, lane);
    }
    wave_fence();
#pragma unroll
    for (int r = 0; r < KREGS; r++) {
      const uint32_t pos = lane * KREGS + r;
      if (pos < w) {
        s_tk[pos] = top.tk[r];
        s_seg[pos] = top.seg[r];
        s_doc[pos] = top.doc[r];
        odoc[pos] = top.doc[r];
        oseg[pos] = top.seg[r];
        oscore[pos] = key_to_float(top.tk[r]);
      }
    }
  }
  __syncthreads();

  // ---- the detail arrays: each row finds its new place (the rows better than it) by binary search ----
#pragma unroll
  for (int r = 0; r < R; r++) {
    const uint32_t i = tid + kRescoreThreads * r;
    if (i >= w) continue;
    const int32_t mtk = total_key(fresh[r]);
    uint32_t lo = 0, hi = w;  // (segment, doc) is unique among a query's rows: exactly `lo` rows are better
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (better<true>(s_tk[mid], s_seg[mid], s_doc[mid], mtk, row_seg[r], doc[r]))
        lo = mid + 1;
      else
        hi = mid;
    }
    ofirst[lo] = first[r];
    orsc[lo] = rsc[r];
    oflag[lo] = matched[r] ? 1u : 0u;
  }
}

inline hipError_t launch_rescore(const RescoreParams &p, int kregs, size_t lds, hipStream_t st) {
  return with_kregs(kregs, [&](auto K) { return launch_with_lds(rescore_kernel<K>, p, p.nq, lds, st); });
}

}  // namespace slg
