// slg_hybrid.hpp — hybrid text + vector search on the device: one request with a text query and `vector`
// clauses (searchlite-core/src/api/reader.rs:2754-2775: collect_vector_maps with require_text_match = true,
// :2379-2469, then merge_vector_hits, :2474-2537).  Per query:
//
//   1. Matched set M: every doc the batch's scoring run left a candidate for and the select kernels accept —
//      not deleted, passes q_filter, passes minimum_should_match where the batch shape supports it
//      (query_eval.matches, :2427-2449, plus passes_root_filter).
//   2. BM25 hits: the top k of M by (score desc, segment asc, doc asc): the batch's own rows, as
//      select_topk_kernel leaves them (slg_kernels.hpp), bit for bit those of slg_batch_prepare_plans.
//   3. Clause lists: every doc of M with a vector in clause c's field scores metric_similarity * boost[q][c]
//      (vectors/mod.rs:107-120, api/reader.rs:2421: cosine = dot, NaN -> 0; L2 = -sqrt(sum d^2)); the best
//      cand_size by (score desc, segment asc, doc asc) form the list.  Exact where the reference searches an
//      HNSW graph, and every predicate applies before the truncation (as slg_vsearch.hpp).
//   4. Union = BM25 hits + all clause lists.  A union doc's bm25 is its score among the BM25 hits, else 0.0
//      (:2496-2500) — also though it matches the text; per clause blended = bm25 (alpha >= 1), vec
//      (alpha <= 0) or blend_scores(bm25, vec, alpha) (:240-246), vec = the clause's missing-vector score
//      (:217-223) when its list lacks the doc; final = sum / n_clauses; the vector score is the sum of the
//      clause scores found.  When every alpha <= 0 a doc found in no list is dropped (:2494,2504).
//   5. Output: the top k_out by (final desc under f32::total_cmp, segment asc, doc asc), the count, and the
//      union size after the drop.  A row that no clause list holds has no vector score (None): it is written
//      as the missing-vector score of clause 0's metric, what slg_rerank_fields_batch writes for such a row.
//
// hy_gather_kernel is step 3's scan: it walks the candidate entries the scoring kernel wrote (the region of
// slice s starts at slice_cbeg[s] and holds slice_ccnt[s] entries), drops what the select kernels drop (the
// same reject bitmaps), finds each doc's row through the clause field's offsets, streams the whole row with
// 16-byte lane loads against the clause vector in LDS, and appends (ordered score << 32 | ~flat), the key of
// slg_vsearch.hpp, to the (query, clause) key area.  vs_select_kernel folds the key area into the clause
// lists and vs_blend_kernel<true> does steps 4 and 5 (slg_vsearch.hpp).
//
// Work distribution: matched counts run from 0 to a whole segment, so a workgroup takes a span of candidate
// SLOTS, not a query: the candidate area is one index space in query order (a sub-query's region is as long
// as its posting lists; the host sizes the grid from that), a workgroup finds the slices that overlap its
// span by a binary search over slice_cbeg, and its waves take the 64-entry batches of those slices in turn.
// A wave scores a batch lane = candidate: for every clause the rows of the lanes that have one are streamed
// four at a time, each lane keeps its own score, and the keys of the batch go out with one ballot and one
// atomic on the (query, clause) count.  Each key is 8 bytes: 8 B x matched docs x clauses of work space.
//
// What the slice search relies on (stated at RoundScoreParams::slice_cbeg, slg_score.hpp): the scoring kernels
// write slice_cbeg and slice_ccnt of EVERY slice, also of one without candidates, and slice_cbeg is
// non-decreasing in the slice index over the whole batch, regions never overlapping.  The select kernels read
// cbeg only together with ccnt and would survive a scoring kernel that skipped an empty slice; this kernel
// would not.  The host checks the order it can see — the sub-queries' region bases, q_cand — when it
// prepares the batch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_wave.hpp"

namespace slg {

constexpr uint32_t kHyThreads = 256;
constexpr uint32_t kHySpanMax = 1024;         // candidate slots of a workgroup: 64 (one wave) .. this
constexpr uint32_t kHyLdsFloats = 36 * 1024;  // a query's clause vectors in LDS (as rerank_fields_kernel's budget)

struct HyClause {
  const VecSegDev *vsegs;  // the clause field's per-segment stores
  uint32_t dim;
  uint32_t lds_off;  // the clause vector in LDS (floats, a multiple of 4)
  uint32_t q_off;    // ... and in the query's row of qvecs
  int32_t metric;
};

struct HyGatherParams {
  const uint2 *cand;  // .x ordered score, .y doc (0xFFFFFFFF: dropped by the select)
  const uint64_t *slice_cbeg;
  const uint32_t *slice_ccnt, *slice_seg, *slice_sq;
  const RoundQuery *sq;
  uint32_t n_slices, n_segs;
  const SegDev *segs;
  const uint32_t *q_filter;             // [nq] 0 = none, f + 1, or nullptr
  const uint32_t *const *reject_table;  // [n_filters * n_segs] reject bitmaps
  const uint32_t *doc_base;             // [n_segs + 1] first flat doc of each segment
  const float *qvecs;                   // query q's clause vectors: qvecs + q * q_stride
  const float *boost;                   // [nq][n_clauses] or nullptr
  uint32_t q_stride, n_clauses, nq, span;
  HyClause cl[8];
  uint64_t slot_lo, slot_hi;  // the candidate slots of this launch (the regions of a range of queries)
  const uint64_t *q_cand;     // [nq + 1] first candidate slot of each query
  uint64_t *keys;             // [clause][slot_hi - slot_lo]: query q's keys from q_cand[q] - slot_lo on
  uint32_t *key_cnt;          // [clause][nq] keys appended
};

// The boosted similarities of the lanes of a wave that `have` a row (row off of `values`) against the clause
// vector at s_qc.  CH > 0: dim <= 256 * CH and dim % 4 == 0, whole rows in 16-byte lane loads, four rows in
// flight; CH == 0: any dimension, 4-byte loads.  L2 is the direct sum (x - y)^2 (slg_vsearch.hpp: the
// expanded form cancels for near-duplicates).
template <int CH>
__device__ __forceinline__ float hy_score_rows(const float *values, const uint32_t dim, const int32_t metric,
                                               const float *s_qc, const uint32_t off, const bool have,
                                               const float bst, const uint32_t lane) {
  float my = 0.0f;
  uint64_t m = __ballot(have);
  if constexpr (CH > 0) {
    constexpr int U = 4;
    typedef const __attribute__((address_space(1))) f32x4_t *grow_t;
    f32x4_t a[CH];
    uint32_t idx[CH];
    bool valid[CH];
#pragma unroll
    for (int ch = 0; ch < CH; ch++) {
      const uint32_t i = ch * 256 + lane * 4;
      valid[ch] = i < dim;
      idx[ch] = valid[ch] ? i : 0u;  // (lanes past the row's end re-read its first floats and are masked out)
      const f32x4_t v = *reinterpret_cast<const f32x4_t *>(s_qc + idx[ch]);
      a[ch] = valid[ch] ? v : (f32x4_t){0.f, 0.f, 0.f, 0.f};
    }
    while (m) {
      uint32_t j[U];
      bool ok[U];
      const uint32_t j_first = (uint32_t)__builtin_ctzll(m);
#pragma unroll
      for (int u = 0; u < U; u++) {  // (a group of fewer than four reads the first row again)
        ok[u] = m != 0ull;
        j[u] = ok[u] ? (uint32_t)__builtin_ctzll(m) : j_first;
        m = ok[u] ? m & (m - 1) : m;
      }
      f32x4_t b[U][CH];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const grow_t row = (grow_t)(values + (size_t)rl(off, j[u]) * dim);
#pragma unroll
        for (int ch = 0; ch < CH; ch++) b[u][ch] = row[idx[ch] >> 2];
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        float acc = 0.0f;
#pragma unroll
        for (int ch = 0; ch < CH; ch++) {
          const f32x4_t bb = valid[ch] ? b[u][ch] : a[ch];  // masked lanes: a = 0 and a - a = 0
          if (metric == 0) {
            acc += a[ch].x * bb.x;
            acc += a[ch].y * bb.y;
            acc += a[ch].z * bb.z;
            acc += a[ch].w * bb.w;
          } else {
            const float d0 = a[ch].x - bb.x, d1 = a[ch].y - bb.y, d2 = a[ch].z - bb.z, d3 = a[ch].w - bb.w;
            acc += d0 * d0;
            acc += d1 * d1;
            acc += d2 * d2;
            acc += d3 * d3;
          }
        }
        const float s = similarity_from_sum(metric, wave_sum_f(acc)) * bst;
        if (ok[u] && lane == j[u]) my = s;
      }
    }
  } else {
    typedef const __attribute__((address_space(1))) float *gf_t;
    while (m) {
      const uint32_t j = (uint32_t)__builtin_ctzll(m);
      m &= m - 1;
      const gf_t row = (gf_t)(values + (size_t)rl(off, j) * dim);
      float acc = 0.0f;
      for (uint32_t i = lane; i < dim; i += 64) {
        const float x = s_qc[i], y = row[i];
        if (metric == 0) {
          acc += x * y;
        } else {
          const float d = x - y;
          acc += d * d;
        }
      }
      const float s = similarity_from_sum(metric, wave_sum_f(acc)) * bst;
      if (lane == j) my = s;
    }
  }
  return my;
}

__global__ void __launch_bounds__(kHyThreads) hy_gather_kernel(HyGatherParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *s_q = reinterpret_cast<float *>(smem);  // the clause vectors of the query at hand
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
  const uint32_t NC = p.n_clauses;
  const uint64_t start = p.slot_lo + (uint64_t)blockIdx.x * p.span;
  const uint64_t end = start + p.span < p.slot_hi ? start + p.span : p.slot_hi;
  if (p.n_slices == 0 || start >= end) return;
  uint32_t lo = 0, hi = p.n_slices;  // the last slice that starts at or before the span
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (p.slice_cbeg[mid] <= start)
      lo = mid;
    else
      hi = mid;
  }
  uint32_t cur_q = 0xFFFFFFFFu, nb = 0;
  uint64_t q_first = 0, q_cap = 0;  // the query's first slot and its slots
  const uint32_t *rej = nullptr;
  for (uint32_t s = lo; s < p.n_slices; s++) {
    const uint64_t cb = p.slice_cbeg[s];
    if (cb >= end) break;
    const uint64_t ce = cb + p.slice_ccnt[s];
    const uint64_t a = cb > start ? cb : start, e = ce < end ? ce : end;
    if (a >= e) continue;
    const uint32_t q = p.sq[p.slice_sq[s]].q, seg = p.slice_seg[s];
    if (q >= p.nq || seg >= p.n_segs) continue;
    if (q != cur_q) {  // (the same for every wave of the workgroup: the slices are walked in step)
      __syncthreads();
      for (uint32_t c = 0; c < NC; c++)
        for (uint32_t i = tid; i < p.cl[c].dim; i += blockDim.x)
          s_q[p.cl[c].lds_off + i] = p.qvecs[(size_t)q * p.q_stride + p.cl[c].q_off + i];
      __syncthreads();
      cur_q = q;
      q_first = p.q_cand[q];
      q_cap = p.q_cand[q + 1] - q_first;
    }
    // what the select kernels drop: the query's filter bitmap (deleted | ~filter), else the tombstones
    const uint32_t flt = p.q_filter ? p.q_filter[q] : 0u;
    rej = flt ? p.reject_table[(size_t)(flt - 1) * p.n_segs + seg] : p.segs[seg].deleted;
    const uint32_t base_flat = p.doc_base[seg];
    const uint32_t n_bat = (uint32_t)((e - a + 63) >> 6);
    for (uint32_t bi = 0; bi < n_bat; bi++) {
      if ((nb + bi) % n_waves != wave) continue;
      const uint64_t at = a + ((uint64_t)bi << 6) + lane;
      uint32_t doc = 0xFFFFFFFFu;
      if (at < e) doc = p.cand[at].y;
      bool live = doc != 0xFFFFFFFFu && doc < p.segs[seg].n_docs;
      if (live && rej) live = ((rej[doc >> 5] >> (doc & 31)) & 1u) == 0u;
      for (uint32_t c = 0; c < NC; c++) {
        const HyClause cl = p.cl[c];
        const VecSegDev vd = cl.vsegs[seg];
        uint32_t off = 0xFFFFFFFFu;
        if (live && vd.dim == cl.dim && doc < vd.n_docs) off = vd.offsets[doc];
        const bool have = off != 0xFFFFFFFFu;
        if (__ballot(have) == 0ull) continue;
        const float bst = p.boost ? p.boost[(size_t)q * NC + c] : 1.0f;
        const float *s_qc = s_q + cl.lds_off;
        float sc;
        if ((cl.dim & 3u) != 0 || cl.dim > 768u)
          sc = hy_score_rows<0>(vd.values, cl.dim, cl.metric, s_qc, off, have, bst, lane);
        else if (cl.dim <= 256u)
          sc = hy_score_rows<1>(vd.values, cl.dim, cl.metric, s_qc, off, have, bst, lane);
        else if (cl.dim <= 512u)
          sc = hy_score_rows<2>(vd.values, cl.dim, cl.metric, s_qc, off, have, bst, lane);
        else
          sc = hy_score_rows<3>(vd.values, cl.dim, cl.metric, s_qc, off, have, bst, lane);
        // one ballot and one atomic per wave and clause
        const uint32_t pos = wave_compact_slot(&p.key_cnt[(size_t)c * p.nq + q], have, lane);
        if (have && pos < q_cap)
          p.keys[(size_t)c * (p.slot_hi - p.slot_lo) + (q_first - p.slot_lo) + pos] =
              ((uint64_t)ordered_score(sc) << 32) | (uint32_t)~(base_flat + doc);
      }
    }
    nb += n_bat;
  }
}

}  // namespace slg
