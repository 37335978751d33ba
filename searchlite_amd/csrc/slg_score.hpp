// slg_score.hpp — shared definitions of the round-scoring kernels: RoundScoreParams, the cut-point
// searches (also used by partition_rounds_kernel, slg_kernels.hpp), wave scans, in-kernel stamps
// (diagnostic builds).
// The scoring kernels themselves: slg_score_uni4.hpp (<= 8 lists), slg_score_multi.hpp (9..32
// lists, score plans beyond the few-term kernel's, MaxScore / block-max pruning).
//
// Restates query/wand.rs:459-566 (brute_force: every posting of every term is scored and
// summed per doc, in ScorePlan leaf order planner.rs:122-135) and push_top_k
// (wand.rs:905-916) for a whole batch of queries.
//
// Work decomposition (built by the host + partition_rounds_kernel):
//   sub-query = (query, segment);  round = a doc-id range of a sub-query holding about one
//   register set of postings over all its lists, with the exact per-list posting ranges known
//   up front;  slice = consecutive rounds owned by ONE WAVE (no workgroup barriers).
// Integer/f32 VALU + LDS work bounded by the HBM stream of postings; no MFMA on this path.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_wave.hpp"

namespace slg {

// (planning constants: slg_desc.hpp)
// per-wave LDS: bitmap words, exclusive prefix popcounts, accumulators

// first index of d[0, df) with d[idx] >= target, looked for in the 16 NP postings from `a` on: NP + 1
// pivots 16 postings apart (independent loads, one latency) bracket it to 16 postings, which are then
// read whole (one more latency) — two dependent loads instead of a bisection's ~8; false if the
// answer lies outside the window.  The list is
// followed by kListPad sentinels (0xFFFFFFFF), so positions up to df + 63 may be read.
template <int NP = 8, typename DocPtr>
__device__ __forceinline__ bool lower_bound_window(const DocPtr d, uint32_t df, uint32_t target, uint32_t a,
                                                   uint32_t &pos) {
  uint32_t below = 0;  // pivots d[a + 16 i - 1], i = 0..NP, that are < target (i = 0 at a == 0: -inf)
#pragma unroll
  for (uint32_t i = 0; i <= (uint32_t)NP; i++) {
    const uint32_t at = a + 16u * i;
    const uint32_t idx = at - 1u < df ? at - 1u : df;  // (past the end: the first sentinel)
    const uint32_t v = d[at == 0u ? 0u : idx];
    below += (at == 0u || v < target) ? 1u : 0u;
  }
  if (below < 1u || below > (uint32_t)NP) return false;
  const uint32_t base = a + 16u * (below - 1u);  // d[base - 1] < target <= d[base + 15]
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t i = 0; i < 16; i++) cnt += d[base + i] < target ? 1u : 0u;
  pos = base + cnt;
  return true;
}

// first index of d[0, df) with d[idx] >= target: the window around the position a uniform doc-id
// distribution predicts (doc ids are validated < n_docs at staging, so the guess is <= df); if the
// guess was off by more than 64 postings, a bracket widened until it holds the answer (64-bit
// width: a list may hold up to 2^32 - 2 postings and w grows by 8x per step), then a bisection
template <typename DocPtr>
__device__ __forceinline__ uint32_t lower_bound_guess(const DocPtr d, uint32_t df, uint32_t target, uint32_t n_docs) {
  uint32_t g = (uint32_t)(((uint64_t)df * target) / (n_docs ? n_docs : 1u));
  g = g < df ? g : df;
  uint32_t lo = 0, hi = df;
  if (lower_bound_window<8>(d, df, target, g > 64u ? g - 64u : 0u, lo)) return lo;
  lo = 0;
  for (uint64_t w = 512; w < df; w <<= 3) {
    const uint32_t a = g > w ? (uint32_t)(g - w) : 0u;
    const uint32_t e = (uint64_t)g + w < df ? (uint32_t)(g + w) : df;
    const bool lo_ok = a == 0u || d[a - 1] < target;   // answer >= a
    const bool hi_ok = e == df || d[e - 1] >= target;  // answer <= e - 1
    if (lo_ok && hi_ok) {
      lo = a;
      hi = e == df ? df : e - 1;
      break;
    }
  }
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (d[mid] < target)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// ---- scoring -----------------------------------------------------------------------------------
struct RoundScoreParams {
  const RoundQuery *sq;
  const TermRef *terms;
  const uint32_t *slice_sq;
  const uint32_t *slice_order;  // [n_slices] wave w runs slice slice_order[w] (most rounds first)
  const SliceDesc *slice_desc;  // [n_slices] by launch position (partition_rounds_kernel)
  const SegDev *segs;
  const uint32_t *bounds;
  const uint32_t *rdoc;
  int32_t *slice_tk;    // [n_slices * k]
  uint32_t *slice_doc;  // [n_slices * k]
  uint32_t *q_scored;   // [nq] or null
  const uint32_t *const *reject_table;  // [n_filters * n_segs] reject bitmaps (doc filters)
  uint32_t n_segs;
  uint32_t plan_batch;  // multi kernel: 1 = some sub-query has a score plan, 2 = a two-level one, 4 = a deeper
                        // tree (acc / max arrays in LDS: this many sets of kMultiPlanLds bytes)
  const PlanNode *plan_nodes;  // canonical node tables of the deep trees (RoundQuery::node_begin)
  // large-k mode of the uniform kernel (k > 256): candidates instead of per-slice top-k lists
  uint2 *cand;            // {ordered score, doc}; sub-query region + posting offset of the slice
  // INVARIANT (hy_gather_kernel, slg_hybrid.hpp, searches this array): every scoring wave writes its slice's
  // slice_cbeg and slice_ccnt, also when it kept no candidate, and slice_cbeg is non-decreasing in the slice
  // index over the whole batch (slices lie per sub-query in query order; cbeg = the sub-query's base + the
  // postings before the slice).  A kernel that leaves early must still store both.
  uint64_t *slice_cbeg;   // [n_slices] first candidate slot of the slice
  uint32_t *slice_ccnt;   // [n_slices] candidates written
  uint32_t n_slices;
  uint32_t k;
  // block skipping (many-term kernel with classified lists): 64-posting slots of non-essential
  // lists whose doc range holds no doc of an essential list are never loaded
  uint32_t block_skip;
  // postings of non-essential lists that were never loaded: [0] of the batch, [1 + q] of query q; or null
  unsigned long long *skip_counts;
  unsigned long long *stamps;  // [n_slices * 8] (SLG_STAMPS builds only)
  uint32_t *error_flag;        // set (non-zero) by a wave that gave up on a round: slg_batch_fetch fails then
};

// inclusive wave scan (sum) with DPP row shifts + row broadcasts (gfx9 DPP controls)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  // row_shr:1,2,3 then 4, 8 within rows of 16; then row_bcast:15 and row_bcast:31
  uint32_t x = v;
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true);   // row_shr:1
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true);   // row_shr:2
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true);   // row_shr:4
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true);   // row_shr:8
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, true);   // row_bcast:15
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, true);   // row_bcast:31
  return x;
}

#ifdef SLG_STAMPS
// diagnostic build only: cycle stamps per phase, summed per wave, stored to a debug buffer
#define SLG_STAMP(i)                                                                        \
  do {                                                                                      \
    unsigned long long _t;                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                      \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");              \
    __builtin_amdgcn_sched_barrier(0);                                                      \
    st_acc[i] += _t - st_last;                                                              \
    st_last = _t;                                                                           \
  } while (0)
#else
#define SLG_STAMP(i) \
  do {               \
  } while (0)
#endif

// shared by the scoring kernels
constexpr int kJoinWords = 1024;  // filter words of the few-term kernels = 8192 doc fields; also the join queue
static_assert(kJoinWords * 4 >= kUniCap * 8, "the join queue ({doc, score} per posting) overlays the filter");
// k <= 256 (KREGS <= 4): buffered top-k in LDS (BufTopK); larger k: every doc above the seed
// threshold goes to the slice's candidate region and select_topk_kernel picks the k best
constexpr bool uni_buffered(int kregs) { return kregs <= 4; }

typedef const __attribute__((address_space(1))) uint32_t *gu32_t;
typedef const __attribute__((address_space(1))) float *gf32_t;

}  // namespace slg
