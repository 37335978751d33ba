// slg_kernels.hpp — hand-written HIP kernels for gfx950 (CDNA4, wave64).
//
// Path restated (reference file:line relative to searchlite-core/src/):
//   stage_impacts   : (slg_stage.hpp)
//   score_rounds    : (slg_score.hpp) query/wand.rs:459-566 + push_top_k :905-916
//   merge_topk      : query/wand.rs:918-926 + api/reader.rs:2776-2778 (query/sort.rs:80-93)
//
// This header: the kernels a batch runs around the scoring kernels — the round partition, the merges
// and the large-k / field-sorted selects.  Only slg_batch.hip includes it (a static kernel is compiled
// into every unit that includes its header); the staging and filter kernels of the index are in
// slg_stage.hpp.  Wave-level helpers (one LDS atomic per wave and bin / per wave and compaction), the
// register top-k with its stream-and-insert loop and its result row: slg_wave.hpp; the scoring kernels:
// slg_score*.hpp.  What the merges and the two selects share beyond that — the error word, the zero fill
// of a short result row, the size of a select's last rank range — is defined once below, ahead of the
// merge kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_desc.hpp"
#include "slg_score.hpp"
#include "slg_wave.hpp"

namespace slg {

// ---- partition: exact per-list cut points of every round --------------------------------------
struct RoundPartParams {
  const RoundQuery *sq;
  const TermRef *terms;
  const SegDev *segs;
  const uint32_t *bnd_coarse;  // [ceil(n_boundaries / 32)] sub-query of every 32nd boundary
  uint32_t n_sq;
  uint32_t *bounds;
  uint32_t *rdoc;
  uint32_t *q_scored;  // [nq] zeroed here (saves a memset node per batch)
  unsigned long long *skip_counts;  // [1 + nq] zeroed here, or null
  const uint32_t *slice_sq;     // [n_slices]
  const uint32_t *slice_order;  // [n_slices] launch position -> slice
  SliceDesc *slice_desc;        // [n_slices] out, by launch position
  uint32_t nq;
  uint32_t n_boundaries;
  uint32_t n_slices;
  uint32_t tpb_shift;  // log2(threads per boundary): 2 when no sub-query has more than 4 lists, else 3
};

// 4 or 8 threads per boundary: thread u handles lists u, u + threads, ...
// (Measured on config 3, where the kernel takes 1.6 ms: it is bound by the HBM lines it fetches —
// with a round's postings of a list inside one or two lines, the cut points of all rounds touch
// every line of every list but the longest, at scattered-access efficiency.  Giving a thread 8
// consecutive boundaries, each searched behind its predecessor, fetches the same lines and was
// slower: 2.2 ms.)
static __global__ void __launch_bounds__(256) partition_rounds_kernel(RoundPartParams p) {
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid < p.nq) p.q_scored[gid] = 0;
  if (gid <= p.nq && p.skip_counts) p.skip_counts[gid] = 0ull;
  if (gid < p.n_slices) {  // the slice record of launch position gid
    const uint32_t slice = p.slice_order[gid];
    const RoundQuery s = p.sq[p.slice_sq[slice]];
    const uint32_t r0 = (slice - s.slice_begin) * s.rounds_per_slice;
    SliceDesc d;
    d.slice = slice;
    d.term_begin = s.term_begin;
    d.bounds_off = s.bounds_begin + r0 * s.n_terms;
    d.rdoc_off = s.rdoc_begin + r0;
    d.n_terms = s.n_terms;
    d.n_rounds = s.n_rounds - r0 < s.rounds_per_slice ? s.n_rounds - r0 : s.rounds_per_slice;
    d.seg = s.seg;
    d.filter = s.filter;
    d.q = s.q;
    d.theta0 = s.theta0;
    d.cand_lo = s.cand_lo;
    d.cand_hi = s.cand_hi;
    d.first_round = r0;
    d.sq_rounds = s.n_rounds;
    d.longest = s.longest;
    {
      const TermRef L = p.terms[s.term_begin + s.longest];
      d.l_df = L.df;
      d.l_off = L.off;
    }
    d.plan = s.plan;
    d.tie = s.tie;
    d.max_init = s.max_init;
    d.n_leaves = s.n_leaves;
    p.slice_desc[gid] = d;
  }
  const uint32_t tpb = 1u << p.tpb_shift;
  const uint32_t b = gid >> p.tpb_shift, u = gid & (tpb - 1u);
  if (b >= p.n_boundaries) return;
  // the sub-query that owns boundary b: the last one whose first boundary is <= b (bnd_begin
  // ascends).  The host uploads it for every 32nd boundary (a per-boundary table was most of the
  // descriptor upload); from there a short walk (sub-queries have ~85 boundaries on config 2)
  uint32_t sqi = p.bnd_coarse[b >> 5];
  while (sqi + 1 < p.n_sq && p.sq[sqi + 1].bnd_begin <= b) sqi++;
  const RoundQuery s = p.sq[sqi];
  const uint32_t j = b - s.bnd_begin;
  const uint32_t *docs = p.segs[s.seg].docs;
  const TermRef L = p.terms[s.term_begin + s.longest];
  const uint32_t stride = (L.df + s.n_rounds - 1) / s.n_rounds;
  const uint64_t posL = (uint64_t)j * stride;
  const bool first = j == 0, last = j >= s.n_rounds || posL >= L.df;
  uint32_t target = 0;
  if (!first && !last) target = docs[L.off + posL];
  for (uint32_t t = u; t < s.n_terms; t += tpb) {
    const TermRef me = p.terms[s.term_begin + t];
    uint32_t out;
    if (first) {
      out = 0;
    } else if (last) {
      out = me.df;
    } else if (t == s.longest) {
      out = (uint32_t)posL;
    } else {
      out = lower_bound_guess(docs + me.off, me.df, target, p.segs[s.seg].n_docs);
    }
    p.bounds[s.bounds_begin + j * s.n_terms + t] = out;
  }
  if (u == 0) {
    uint32_t rd;
    if (first) {  // smallest first doc over the lists
      rd = 0xFFFFFFFFu;
      for (uint32_t t = 0; t < s.n_terms; t++) {
        const TermRef me = p.terms[s.term_begin + t];
        const uint32_t d0 = docs[me.off];
        rd = d0 < rd ? d0 : rd;
      }
    } else if (last) {  // one past the largest last doc
      rd = 0;
      for (uint32_t t = 0; t < s.n_terms; t++) {
        const TermRef me = p.terms[s.term_begin + t];
        const uint32_t d1 = docs[me.off + me.df - 1] + 1u;
        rd = d1 > rd ? d1 : rd;
      }
    } else {
      rd = target;
    }
    p.rdoc[s.rdoc_begin + j] = rd;
  }
}

// ---- pieces shared by the merge and select kernels ------------------------------------------------
// The index's error word is copied behind the result block (MergeParams::error_flag) by one thread of the grid.
template <typename P>
__device__ __forceinline__ void copy_error_flag(const P &p, const bool first_thread) {
  if (first_thread && p.out_flag) *p.out_flag = *p.error_flag;
}
// zero the entries [from, k) of query q's result row; thread t of nt
__device__ __forceinline__ void zero_rows(uint32_t *out_doc, uint32_t *out_seg, float *out_score, const uint32_t q,
                                          const uint32_t k, const uint32_t from, const uint32_t t, const uint32_t nt) {
  for (uint32_t i = from + t; i < k; i += nt) {
    out_doc[(size_t)q * k + i] = 0u;
    out_seg[(size_t)q * k + i] = 0u;
    out_score[(size_t)q * k + i] = 0.0f;
  }
}
// The final rank range of a select may take more keys than it emits (dropped after the sort) as long as
// they fit the sort, whose size is the next power of two: no more than that of the `left` keys still to
// emit (k = 1001: a 1024-key sort; up to 2048 keys were 66 stages x 2 passes against 55 x 1), at most cap.
__device__ __forceinline__ uint32_t last_range_cap(const uint32_t left, const uint32_t cap) {
  uint32_t cap_last = 64;
  while (cap_last < left) cap_last <<= 1;
  return cap_last < cap ? cap_last : cap;
}

// ---- merge: per query, all slice candidate lists -> final top-k ---------------------------
struct MergeParams {
  const QueryRef *queries;
  const uint32_t *slice_seg;  // [n_slices] segment ordinal of each slice
  const int32_t *slice_tk;
  const uint32_t *slice_doc;
  uint32_t *out_doc;
  uint32_t *out_seg;
  float *out_score;
  uint32_t *out_count;
  uint32_t nq;
  uint32_t k;
  // the index's error word (a scoring wave that gave up on a round sets it) is copied behind the result
  // block, so that slg_batch_fetch reads it with the results: ONE device-to-host copy per batch
  const uint32_t *error_flag;
  uint32_t *out_flag;
};

// One wave per query.  The query's slices occupy a contiguous range of the candidate arrays
// ([slice_begin*k, slice_end*k)); it is streamed 64 entries at a time (independent coalesced
// loads), filtered against the running threshold and inserted into the register top-k.
template <int KREGS>
__global__ void __launch_bounds__(256) merge_topk_kernel(MergeParams p) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t q = rfl(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  if (q >= p.nq) return;
  copy_error_flag(p, q == 0 && lane == 0);
  const uint32_t k = p.k;
  const QueryRef qr = p.queries[q];
  WaveTopK<KREGS, true> top;
  top.init();
  // candidate arrays are indexed slice*k + i; the host guarantees n_slices*k < 2^32
  const uint32_t f0 = qr.slice_begin * k, f1 = qr.slice_end * k;
  // Several groups of 64 entries (8; 4 in the wide instantiations) are loaded at once and then inserted one after the other: the loop is bound
  // by the latency of its loads (a group's three loads, then a ballot that depends on them: 4.2 us per
  // group with one group in flight — config 3's 110 groups per query made this kernel 0.74 ms, 0.48 of
  // it without a single insert)
  constexpr int G = KREGS <= 4 ? 8 : 4;
  for (uint32_t base = f0; base < f1; base += 64 * G) {
    int32_t gtk[G];
    uint32_t gdoc[G], gseg[G];
#pragma unroll
    for (int u = 0; u < G; u++) {
      const uint32_t f = base + 64u * u + lane;
      gtk[u] = kSentinelTk;
      gdoc[u] = 0xFFFFFFFFu;
      gseg[u] = 0xFFFFFFFFu;
      if (f < f1) {
        gtk[u] = p.slice_tk[f];
        gdoc[u] = p.slice_doc[f];
        gseg[u] = p.slice_seg[f / k];
      }
    }
#pragma unroll
    for (int u = 0; u < G; u++) {
      const int32_t ctk = gtk[u];
      const uint32_t cdoc = gdoc[u], cseg = gseg[u];
      const bool valid = !(ctk == kSentinelTk && cdoc == 0xFFFFFFFFu);
      // (WaveTopK::offer written out: through the member the KREGS = 16 instantiation takes 101 VGPRs, with
      //  this copy 70; the parent commit's took 100)
      uint64_t m = __ballot(valid && top.passes(ctk, cseg, cdoc));
      while (m) {
        const uint32_t l = (uint32_t)__builtin_ctzll(m);
        top.insert((int32_t)rl((uint32_t)ctk, l), rl(cseg, l), rl(cdoc, l), k, lane);
        m &= m - 1;
        m &= __ballot(top.passes(ctk, cseg, cdoc));
      }
    }
  }
  top.store_row(p.out_doc, p.out_seg, p.out_score, p.out_count, q, k, lane);
}

// ---- merge of per-shard results gathered over RCCL (api/reader.rs:2776-2778 across shards) --
// (ShardMergeParams: slg_desc.hpp — the shard unit of the host fills it without this header)

template <int KREGS>
__global__ void __launch_bounds__(256) merge_shards_kernel(ShardMergeParams p) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t q = rfl(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  if (q >= p.nq) return;
  const uint32_t k = p.k;
  WaveTopK<KREGS, true> top;
  top.init();
  for (uint32_t sh = 0; sh < p.n_shards; sh++) {
    const size_t row = (size_t)sh * p.arr_stride + (size_t)q * k;
    const uint32_t cnt = rfl(p.count[(size_t)sh * p.cnt_stride + q]);
    for (uint32_t base = 0; base < cnt; base += 64) {
      const uint32_t i = base + lane;
      int32_t ctk = kSentinelTk;
      uint32_t cdoc = 0xFFFFFFFFu, cseg = 0xFFFFFFFFu;
      if (i < cnt) {
        ctk = total_key(p.score[row + i]);
        cdoc = p.doc[row + i];
        cseg = sh * p.seg_stride + p.seg[row + i];
      }
      // (not WaveTopK::offer: a shard's row is sorted, so the row is left at the first 64 entries that add
      //  nothing, and only the chosen lane is re-tested — the lanes behind it are worse and fall out one
      //  scalar compare each, without a wave-wide ballot per insert.  No single-card workload times this
      //  kernel, so its loop is kept as it was measured.)
      uint64_t m = __ballot(i < cnt && top.passes(ctk, cseg, cdoc));
      if (m == 0) break;
      while (m) {
        const uint32_t l = (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        const int32_t c_tk = (int32_t)rl((uint32_t)ctk, l);
        const uint32_t c_doc = rl(cdoc, l), c_seg = rl(cseg, l);
        if (!top.passes(c_tk, c_seg, c_doc)) continue;
        top.insert(c_tk, c_seg, c_doc, k, lane);
      }
    }
  }
  top.store_row(p.out_doc, p.out_seg, p.out_score, p.out_count, q, k, lane);
}

// ---- the same merge for k beyond the register top-k (k up to 20 001, api/reader.rs:2615-2619) --
// Every shard's row is already sorted by (score desc, segment asc, doc asc) and keys are unique,
// so the global rank of an entry = its own index + the number of better entries in every other
// shard's row (a binary search each); entries ranked below k write themselves to out[rank].
// One workgroup per query.
static __global__ void __launch_bounds__(256) merge_shards_large_kernel(ShardMergeParams p) {
  const uint32_t q = blockIdx.x;
  if (q >= p.nq) return;
  const uint32_t k = p.k;
  uint32_t total = 0;
  for (uint32_t sh = 0; sh < p.n_shards; sh++) {
    const uint32_t c = p.count[(size_t)sh * p.cnt_stride + q];
    total += c < k ? c : k;
  }
  const uint32_t nout = total < k ? total : k;
  for (uint32_t e = threadIdx.x; e < p.n_shards * k; e += blockDim.x) {
    const uint32_t sh = e / k, i = e % k;
    const uint32_t cnt_s = p.count[(size_t)sh * p.cnt_stride + q] < k ? p.count[(size_t)sh * p.cnt_stride + q] : k;
    if (i >= cnt_s) continue;
    const size_t row = (size_t)sh * p.arr_stride + (size_t)q * k;
    const int32_t tk = total_key(p.score[row + i]);
    const uint32_t doc = p.doc[row + i], seg = sh * p.seg_stride + p.seg[row + i];
    uint32_t rank = i;
    for (uint32_t t = 0; t < p.n_shards; t++) {
      if (t == sh) continue;
      const size_t rt = (size_t)t * p.arr_stride + (size_t)q * k;
      uint32_t lo = 0, hi = p.count[(size_t)t * p.cnt_stride + q] < k ? p.count[(size_t)t * p.cnt_stride + q] : k;
      while (lo < hi) {  // first entry of shard t that is NOT better than mine
        const uint32_t mid = (lo + hi) >> 1;
        if (better<true>(total_key(p.score[rt + mid]), t * p.seg_stride + p.seg[rt + mid], p.doc[rt + mid], tk, seg, doc))
          lo = mid + 1;
        else
          hi = mid;
      }
      rank += lo;
    }
    if (rank < k) {
      p.out_doc[(size_t)q * k + rank] = doc;
      p.out_seg[(size_t)q * k + rank] = seg;
      p.out_score[(size_t)q * k + rank] = p.score[row + i];
    }
  }
  zero_rows(p.out_doc, p.out_seg, p.out_score, q, k, nout, threadIdx.x, blockDim.x);
  if (threadIdx.x == 0) p.out_count[q] = nout;
}

// ---- large k (k > 256): per-query radix select over the candidates the scoring kernel kept ----
// The uniform scoring kernel, instead of keeping a per-slice top-k, writes every doc whose score
// beats the seed threshold to its slice's region of `cand` ({ordered score, doc}; the region of
// slice s starts at slice_cbeg[s] and holds slice_ccnt[s] entries).  One workgroup per query
// then finds the k best under (score desc, segment asc, doc asc) = the 96-bit key
// (ordered score, ~segment, ~doc) descending: byte-wise MSB-first radix select with an LDS
// histogram (a pass per byte until the bucket that holds the k-th key is exactly used up), a
// gather of the k winners into LDS and a bitonic sort.  push_top_k / finalize_heap
// (query/wand.rs:905-926) + the cross-segment sort (api/reader.rs:2776-2778) for large k.
// The CURSOR instantiation (slg_batch_prepare_after in score order) also drops, in sweep 1, every candidate
// whose key is at or above the query's cursor key — a hit of an earlier page (api/reader.rs:3009-3036) —
// the way a deleted one is dropped, counts the rest (out_matched) and raises out_seen on the cursor's own key.
struct SelectParams {
  const QueryRef *queries;
  const uint32_t *slice_seg;
  const uint64_t *slice_cbeg;
  const uint32_t *slice_ccnt;
  uint2 *cand;  // .x ordered score, .y doc (0xFFFFFFFF: dropped, e.g. deleted)
  const SegDev *segs;
  const uint32_t *q_filter;             // [nq] 0 = none, f + 1
  const uint32_t *const *reject_table;  // [n_filters * n_segs] reject bitmaps
  uint32_t n_segs;
  uint32_t *out_doc, *out_seg;
  float *out_score;
  uint32_t *out_count;
  uint32_t nq, k;
  const uint32_t *error_flag;  // see MergeParams
  uint32_t *out_flag;
  // (CURSOR only)
  const uint32_t *cursor;            // [nq * kCursorStride]: has_cursor, ordered score, ~segment, ~doc
  unsigned long long *out_matched;   // [nq] accepted docs after the cursor
  uint32_t *out_seen;                // [nq] 1: an accepted doc has the cursor's key (or no cursor)
};

// words per query of a cursor batch's device cursor table: has_cursor, then the key words the select kernel
// compares (select_topk_kernel: 3; select_sorted_kernel: kSortWords)
constexpr uint32_t kCursorStride = 16;

constexpr uint32_t kSelectCap = 2048;      // keys sorted in LDS at a time (a rank range of the result)
constexpr uint32_t kSelectMaxSlices = 512;   // slice table in LDS; more: strided slice loops (34 KB of LDS per workgroup: 4 per CU)
constexpr uint32_t kSelectThreads = 512;

// (8 waves per SIMD: four 512-thread workgroups per CU, so that the 1024 queries of a batch are all resident at once)
template <bool CURSOR>
static __global__ void __launch_bounds__(kSelectThreads) __attribute__((amdgpu_waves_per_eu(8, 8)))
select_topk_kernel(SelectParams p) {
  constexpr uint32_t NT = kSelectThreads;
  __shared__ uint32_t hist[256], hist0[256];  // hist0: top score byte of all live candidates
  __shared__ uint32_t w_ok[kSelectCap], w_sg[kSelectCap], w_dc[kSelectCap];
  __shared__ uint32_t sh_pre[3], sh_need, sh_done, sh_nvalid, sh_nwin, sh_anydel, sh_taken;
  __shared__ uint32_t t_end[kSelectMaxSlices];   // inclusive prefix of the slice counts
  __shared__ uint32_t t_nseg[kSelectMaxSlices];  // ~segment of the slice
  __shared__ uint64_t t_base[kSelectMaxSlices];  // first candidate slot of the slice
  __shared__ uint32_t s_cur[4], sh_seen;          // (CURSOR) the query's cursor words; its key was seen
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t q = blockIdx.x;
  if (q >= p.nq) return;
  copy_error_flag(p, q == 0 && tid == 0);
  const uint32_t k = p.k;
  const QueryRef qr = p.queries[q];
  const uint32_t sb = qr.slice_begin, se = qr.slice_end, nsl = se - sb;
  const bool table = nsl <= kSelectMaxSlices;
  const uint32_t flt = p.q_filter ? p.q_filter[q] : 0u;

  if (tid == 0) {
    sh_nvalid = 0;
    sh_nwin = 0;
    sh_anydel = table ? 0u : 1u;
    sh_pre[0] = sh_pre[1] = sh_pre[2] = 0;
    sh_need = k;
    sh_done = 0;
    sh_taken = 0;
  }
  if (tid < 256) hist0[tid] = 0;
  if constexpr (CURSOR) {
    if (tid < 4) s_cur[tid] = p.cursor[(size_t)q * kCursorStride + tid];
    if (tid == 0) sh_seen = 0;
  }
  __syncthreads();
  // slice table: the query's candidates form one flat index space [0, n)
  if (table) {
    for (uint32_t i = tid; i < nsl; i += NT) {
      const uint32_t sg = p.slice_seg[sb + i];
      t_end[i] = p.slice_ccnt[sb + i];
      t_base[i] = p.slice_cbeg[sb + i];
      t_nseg[i] = ~sg;
      if (p.segs[sg].deleted || flt) sh_anydel = 1;
    }
    __syncthreads();
    for (uint32_t d = 1; d < nsl; d <<= 1) {  // Hillis-Steele inclusive scan
      uint32_t add[kSelectMaxSlices / NT];
      for (uint32_t i = tid, r = 0; i < nsl; i += NT, r++) add[r] = i >= d ? t_end[i - d] : 0u;
      __syncthreads();
      for (uint32_t i = tid, r = 0; i < nsl; i += NT, r++) t_end[i] += add[r];
      __syncthreads();
    }
  }
  __syncthreads();
  const uint32_t n_flat = table && nsl ? t_end[nsl - 1] : 0u;
  const bool anydel = sh_anydel != 0;
  const bool cur_on = CURSOR && s_cur[0] != 0u;
  const uint32_t cur_a = CURSOR ? s_cur[1] : 0u, cur_nseg = CURSOR ? s_cur[2] : 0u, cur_ndoc = CURSOR ? s_cur[3] : 0u;

  // visit every live candidate of the query: f(ordered score, ~seg, ~doc, slot)
  auto for_each = [&](auto &&f) {
    if (table) {
      // (four named sets, not arrays: with arrays the compiler keeps the loop over them rolled around the
      //  inlined callback and the arrays in scratch memory — a scratch round trip per candidate)
      auto locate = [&](const uint32_t i, uint2 &c, uint64_t &at, uint32_t &ns) {
        c = make_uint2(0u, 0xFFFFFFFFu);
        at = 0;
        ns = 0;
        if (i < n_flat) {
          uint32_t lo = 0, hi = nsl - 1;  // first slice whose inclusive prefix exceeds i
          while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (t_end[mid] > i)
              hi = mid;
            else
              lo = mid + 1;
          }
          at = t_base[lo] + (i - (lo ? t_end[lo - 1] : 0u));
          ns = t_nseg[lo];
          c = p.cand[at];
        }
      };
      // eight independent loads in flight per thread: the kernel's time is the time of the query with the
      // most candidates (all workgroups are resident at once), and its sweeps are latency-bound
      for (uint32_t i0 = tid; i0 < n_flat; i0 += 8 * NT) {
        uint2 c0, c1, c2, c3, c4, c5, c6, c7;
        uint64_t a0, a1, a2, a3, a4, a5, a6, a7;
        uint32_t n0, n1, n2, n3, n4, n5, n6, n7;
        locate(i0, c0, a0, n0);
        locate(i0 + NT, c1, a1, n1);
        locate(i0 + 2 * NT, c2, a2, n2);
        locate(i0 + 3 * NT, c3, a3, n3);
        locate(i0 + 4 * NT, c4, a4, n4);
        locate(i0 + 5 * NT, c5, a5, n5);
        locate(i0 + 6 * NT, c6, a6, n6);
        locate(i0 + 7 * NT, c7, a7, n7);
        if (c0.y != 0xFFFFFFFFu) f(c0.x, n0, ~c0.y, a0);
        if (c1.y != 0xFFFFFFFFu) f(c1.x, n1, ~c1.y, a1);
        if (c2.y != 0xFFFFFFFFu) f(c2.x, n2, ~c2.y, a2);
        if (c3.y != 0xFFFFFFFFu) f(c3.x, n3, ~c3.y, a3);
        if (c4.y != 0xFFFFFFFFu) f(c4.x, n4, ~c4.y, a4);
        if (c5.y != 0xFFFFFFFFu) f(c5.x, n5, ~c5.y, a5);
        if (c6.y != 0xFFFFFFFFu) f(c6.x, n6, ~c6.y, a6);
        if (c7.y != 0xFFFFFFFFu) f(c7.x, n7, ~c7.y, a7);
      }
    } else {
      for (uint32_t s = sb + wave; s < se; s += NT / 64) {
        const uint64_t base = p.slice_cbeg[s];
        const uint32_t cnt = p.slice_ccnt[s];
        const uint32_t nseg = ~p.slice_seg[s];
        for (uint32_t i = lane; i < cnt; i += 64) {
          const uint2 c = p.cand[base + i];
          if (c.y != 0xFFFFFFFFu) f(c.x, nseg, ~c.y, base + i);
        }
      }
    }
  };

  // ---- sweep 1: accept() (drop deleted docs) + histogram of the top score byte ----
  for_each([&](uint32_t a, uint32_t nseg, uint32_t ndoc, uint64_t at) {
    if (anydel) {
      const uint32_t *del = flt ? p.reject_table[(size_t)(flt - 1) * p.n_segs + ~nseg] : p.segs[~nseg].deleted;
      const uint32_t d = ~ndoc;
      if (del && ((del[d >> 5] >> (d & 31)) & 1u)) {
        p.cand[at].y = 0xFFFFFFFFu;
        return;
      }
    }
    if constexpr (CURSOR) {  // (descending key: at or above the cursor's = SortKey <= the cursor's)
      if (cur_on && (a > cur_a || (a == cur_a && (nseg > cur_nseg || (nseg == cur_nseg && ndoc >= cur_ndoc))))) {
        if (a == cur_a && nseg == cur_nseg && ndoc == cur_ndoc) sh_seen = 1u;
        p.cand[at].y = 0xFFFFFFFFu;
        return;
      }
    }
    // (scores of one query share their exponent: nearly all candidates fall into one or two bins, and LDS
    //  atomics on one address are served one at a time — 2K of them were 27 us of this kernel.  The
    //  lanes of a wave that hold the same bin add their count once.)
    hist_add_by_bin(hist0, a >> 24, lane);
  });
  __syncthreads();
  if (wave == 0) {  // (one wave adds the 256 bins: a single thread walking them was ~10 us of this kernel)
    uint32_t nv = hist0[4 * lane] + hist0[4 * lane + 1] + hist0[4 * lane + 2] + hist0[4 * lane + 3];
    for (int o = 32; o > 0; o >>= 1) nv += __shfl_xor(nv, o, 64);
    if (lane == 0) sh_nvalid = nv;
  }
  __syncthreads();
  const uint32_t nvalid = sh_nvalid;
  const uint32_t nout = nvalid < k ? nvalid : k;

  // decided-prefix compare: key (a, b, c) >= prefix (p0, p1, p2) on the top (level + 1) bytes
  auto at_or_above = [](uint32_t a, uint32_t b, uint32_t c, uint32_t p0, uint32_t p1, uint32_t p2,
                        uint32_t level) {
    const uint32_t wd = level >> 2, shift = 24u - 8u * (level & 3u);
    const uint32_t keep = ~((1u << shift) - 1u);  // decided bytes of word wd
    const uint32_t ka = wd == 0 ? (a & keep) : a, kb = wd == 1 ? (b & keep) : b,
                   kc = wd == 2 ? (c & keep) : c;
    if (wd == 0) return ka >= p0;
    if (wd == 1) return ka > p0 || (ka == p0 && kb >= p1);
    return ka > p0 || (ka == p0 && (kb > p1 || (kb == p1 && kc >= p2)));
  };

  // ---- the result is produced in rank ranges of at most kSelectCap keys: for each range a
  //      byte-wise radix select finds the prefix of its last key (exactly, except for the final
  //      range, which may take a few keys more than needed and drops them after the sort), the
  //      keys between this prefix and the previous range's are gathered, sorted, written ----
  uint32_t k_done = 0;
  bool have_prev = false;
  uint32_t q0 = 0, q1 = 0, q2 = 0, q_level = 0;  // prefix of the previous range
  while (k_done < nout) {
    const uint32_t target = nout - k_done > kSelectCap ? k_done + kSelectCap : nout;
    const bool last = target == nout;
    uint32_t cap_last = last_range_cap(nout - k_done, kSelectCap);
    if (n_flat > 16u * NT) cap_last = kSelectCap;  // (many candidates: a further select level costs more than the larger sort)
    const bool all = last && nvalid - k_done <= cap_last;  // everything left fits: no select
    __syncthreads();
    if (tid == 0) {
      sh_pre[0] = sh_pre[1] = sh_pre[2] = 0;
      sh_need = target;
      sh_done = all ? 2u : 0u;
      sh_taken = all ? nvalid : 0u;
      sh_nwin = 0;
    }
    __syncthreads();
    uint32_t level = 0;
    if (!all) {
      for (;; level++) {
        const uint32_t wd = level >> 2, shift = 24u - 8u * (level & 3u);
        if (tid < 256) hist[tid] = level == 0 ? hist0[tid] : 0u;
        __syncthreads();
        if (level > 0) {
          const uint32_t p0 = sh_pre[0], p1 = sh_pre[1], p2 = sh_pre[2];
          const uint32_t himask = shift == 24u ? 0u : ~((1u << (shift + 8u)) - 1u);  // bytes above
          for_each([&](uint32_t a, uint32_t b, uint32_t c, uint64_t) {
            const uint32_t w = wd == 0 ? a : (wd == 1 ? b : c), pw = wd == 0 ? p0 : (wd == 1 ? p1 : p2);
            bool m = (w & himask) == (pw & himask);
            if (wd >= 1) m = m && a == p0;
            if (wd >= 2) m = m && b == p1;
            if (m) atomicAdd(&hist[(w >> shift) & 255u], 1u);
          });
          __syncthreads();
        }
        if (wave == 0) {
          // lane l owns bins 255-4l .. 252-4l (descending); inclusive prefix of the lane sums
          // (select_sorted_kernel has the ascending twin of this pick: folded into one helper templated on the
          //  direction, in two forms, it cost that kernel 4 to 6 VGPRs above its 141)
          const uint32_t b0 = 255u - 4u * lane;
          const uint32_t h0 = hist[b0], h1 = hist[b0 - 1], h2 = hist[b0 - 2], h3 = hist[b0 - 3];
          const uint32_t tot = h0 + h1 + h2 + h3;
          uint32_t incl = tot;
          for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(incl, o, 64);
            if ((int)lane >= o) incl += v;
          }
          const uint32_t need = sh_need, excl = incl - tot;
          if (excl < need && need <= incl) {  // exactly one lane (need <= matching keys)
            uint32_t cum = excl, b = b0, h = h0;
            if (cum + h < need) { cum += h; b = b0 - 1; h = h1; }
            if (cum + h < need) { cum += h; b = b0 - 2; h = h2; }
            if (cum + h < need) { cum += h; b = b0 - 3; h = h3; }
            sh_pre[wd] = sh_pre[wd] | (b << shift);
            sh_need = need - cum;  // rank of the target key inside the bucket
            const uint32_t taken = (target - (need - cum)) + h;  // keys with prefix >= the chosen one
            sh_taken = taken;
            // exact when the whole bucket is wanted; the final range may overshoot within the buffer
            sh_done = (h == need - cum || level == 11 || (last && taken - k_done <= cap_last)) ? 1u : 0u;
          }
        }
        __syncthreads();
        if (sh_done) break;
      }
    }
    const uint32_t p0 = sh_pre[0], p1 = sh_pre[1], p2 = sh_pre[2];
    const uint32_t count = (sh_taken - k_done) < kSelectCap ? (sh_taken - k_done) : kSelectCap;
    // ---- gather the keys of this range ----
    for_each([&](uint32_t a, uint32_t b, uint32_t c, uint64_t) {
      bool win = all || at_or_above(a, b, c, p0, p1, p2, level);
      if (win && have_prev) win = !at_or_above(a, b, c, q0, q1, q2, q_level);
      const uint32_t at = wave_compact_slot(&sh_nwin, win, lane);  // (one add per wave: see the histogram above)
      if (win && at < kSelectCap) {
        w_ok[at] = a;
        w_sg[at] = b;
        w_dc[at] = c;
      }
    });
    __syncthreads();
    // ---- bitonic sort, descending 96-bit key ----
    uint32_t n2 = 1;
    while (n2 < count) n2 <<= 1;
    for (uint32_t i = count + tid; i < n2; i += NT) {
      w_ok[i] = 0;
      w_sg[i] = 0;
      w_dc[i] = 0;
    }
    __syncthreads();
    for (uint32_t size = 2; size <= n2; size <<= 1) {
      for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
        for (uint32_t t = tid; t < (n2 >> 1); t += NT) {
          const uint32_t i = 2 * t - (t & (stride - 1));  // lower index of the pair
          const uint32_t j = i + stride;
          const bool desc = (i & size) == 0;
          const uint32_t ai = w_ok[i], bi = w_sg[i], ci = w_dc[i];
          const uint32_t aj = w_ok[j], bj = w_sg[j], cj = w_dc[j];
          const bool i_lt_j = ai < aj || (ai == aj && (bi < bj || (bi == bj && ci < cj)));
          if (i_lt_j == desc) {
            w_ok[i] = aj; w_sg[i] = bj; w_dc[i] = cj;
            w_ok[j] = ai; w_sg[j] = bi; w_dc[j] = ci;
          }
        }
        __syncthreads();
      }
    }
    const uint32_t emit = target - k_done;  // (the final range drops what it took beyond k)
    for (uint32_t i = tid; i < emit; i += NT) {
      const int32_t tk = (int32_t)(w_ok[i] ^ 0x80000000u);
      p.out_doc[(size_t)q * k + k_done + i] = ~w_dc[i];
      p.out_seg[(size_t)q * k + k_done + i] = ~w_sg[i];
      p.out_score[(size_t)q * k + k_done + i] = key_to_float(tk);
    }
    k_done = target;
    have_prev = true;
    q0 = p0;
    q1 = p1;
    q2 = p2;
    q_level = level;
  }
  zero_rows(p.out_doc, p.out_seg, p.out_score, q, k, nout, tid, NT);
  if (tid == 0) p.out_count[q] = nout;
  if constexpr (CURSOR) {
    if (tid == 0) {
      p.out_matched[q] = nvalid;
      p.out_seen[q] = cur_on ? sh_seen : 1u;
    }
  }
}

// ---- field-sorted select (slg_batch_prepare_sorted; query/sort.rs:80-123 SortKey::cmp) -------------
// A sorted batch runs its scoring kernel in candidates mode without a threshold seed, so every matched doc
// of every sub-query is in the candidate region once with its exact score.  One workgroup per query then
// takes the k smallest composite keys
//   part 0 | part 1 | ... | segment | doc        (ascending u32 words, kSortWords of them)
// where a field part is three words (missing flag, u64 key: the column of its order, complemented for
// Desc on the host, so ascending is the sort order in both; Missing = flag 1, sorts last in both orders)
// and a `_score` part is the ordered score (complemented for Desc) in the third word of its three.
// Parts beyond the spec are zero words.  Keys are regathered from the columns on every sweep (L2), never
// held per candidate.  Sweep 1 applies accept() (tombstones / filter, counted for `matched`) and finds
// which key bytes vary over the query's candidates; the byte-wise radix select (as select_topk_kernel's:
// rank ranges of at most kSortedCap keys, a pass per VARYING byte until the bucket of the range's last
// key is used up) then walks those bytes only.  A range's keys are gathered into LDS — only their
// varying words — and bitonic-sorted by index.  The CURSOR instantiation (slg_batch_prepare_after with a
// sort spec) drops in sweep 1 every accepted candidate whose key is <= the query's cursor key (the words of
// kSortWords the host encoded from the cursor's values) as it drops a deleted one, so neither `matched` nor
// the radix levels see it, and raises out_seen on an equal key.  (SortColDev, kSortMaxParts, kSortWords:
// slg_desc.hpp; the key itself: slg_wave.hpp sorted_key)
struct SortedSelectParams {
  const QueryRef *queries;
  const uint32_t *slice_seg;
  const uint64_t *slice_cbeg;
  const uint32_t *slice_ccnt;
  uint2 *cand;  // .x ordered score, .y doc (0xFFFFFFFF: dropped)
  const SegDev *segs;
  const uint32_t *q_filter;             // [nq] 0 = none, f + 1
  const uint32_t *const *reject_table;  // [n_filters * n_segs] reject bitmaps
  const SortColDev *sort_cols;          // [kSortMaxParts * n_segs]: part p of segment s at p * n_segs + s
  uint32_t n_segs, n_parts;
  uint32_t score_parts;  // bit p: part p is `_score`
  uint32_t desc_parts;   // bit p: part p descends (applied here to `_score`; field columns come complemented)
  uint32_t *out_doc, *out_seg;
  float *out_score;
  uint32_t *out_count;
  unsigned long long *out_matched;  // [nq] accepted docs (total_matches)
  uint32_t nq, k;
  const uint32_t *error_flag;  // see MergeParams
  uint32_t *out_flag;
  // (CURSOR only)
  const uint32_t *cursor;  // [nq * kCursorStride]: has_cursor, then the kSortWords key words
  uint32_t *out_seen;      // [nq] 1: an accepted doc has the cursor's key (or no cursor)
};

constexpr uint32_t kSortedCap = 1024;  // keys sorted in LDS at a time (their varying words: <= 56 KB)
constexpr uint32_t kSortedThreads = 512;

// lexicographic compare of (K & mask) with a prefix: -1 below, 0 equal, 1 above
__device__ __forceinline__ int sorted_cmp(const uint32_t (&K)[kSortWords], const uint32_t *pre, const uint32_t *dm) {
  int c = 0;
#pragma unroll
  for (uint32_t w = 0; w < kSortWords; w++) {
    const uint32_t x = K[w] & dm[w], y = pre[w];
    if (c == 0) c = x < y ? -1 : (x > y ? 1 : 0);
  }
  return c;
}

// (no amdgpu_waves_per_eu: capped at 128 VGPRs for two workgroups per CU — what its 60 KB of LDS would
//  allow — it spills 5 VGPRs; uncapped it takes 141 and none, one workgroup per CU)
template <bool CURSOR>
static __global__ void __launch_bounds__(kSortedThreads) select_sorted_kernel(SortedSelectParams p) {
  constexpr uint32_t NT = kSortedThreads, NW = kSortWords, CAP = kSortedCap;
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_and[NW], s_or[NW], s_slot[NW];  // s_slot: LDS row of a varying word, ~0u: constant
  __shared__ uint32_t s_pre[NW], s_dm[NW], s_qpre[NW], s_qdm[NW];  // prefix (and decided bytes) of this / the previous range
  __shared__ uint32_t w_key[NW * CAP];
  __shared__ uint16_t w_idx[CAP];
  __shared__ uint32_t sh_nvalid, sh_nvary, sh_need, sh_done, sh_taken, sh_nwin;
  __shared__ uint32_t s_cur[NW + 1], sh_seen;  // (CURSOR) has_cursor + the cursor's key words; its key was seen
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t q = blockIdx.x;
  if (q >= p.nq) return;
  copy_error_flag(p, q == 0 && tid == 0);
  const uint32_t k = p.k;
  const QueryRef qr = p.queries[q];
  const uint32_t sb = qr.slice_begin, se = qr.slice_end;
  const uint32_t flt = p.q_filter ? p.q_filter[q] : 0u;
  if (tid < NW) {
    s_and[tid] = 0xFFFFFFFFu;
    s_or[tid] = 0u;
    s_qpre[tid] = s_qdm[tid] = 0u;
  }
  if (tid == 0) sh_nvalid = 0;
  if constexpr (CURSOR) {
    if (tid < NW + 1) s_cur[tid] = p.cursor[(size_t)q * kCursorStride + tid];
    if (tid == 0) sh_seen = 0;
  }
  __syncthreads();
  const bool cur_on = CURSOR && s_cur[0] != 0u;

  // visit every live candidate of the query: f(ordered score, segment, doc, slot); a wave per slice
  auto for_each = [&](auto &&f) {
    for (uint32_t s = sb + wave; s < se; s += NT / 64) {
      const uint64_t base = p.slice_cbeg[s];
      const uint32_t cnt = p.slice_ccnt[s];
      const uint32_t seg = p.slice_seg[s];
      for (uint32_t i = lane; i < cnt; i += 64) {
        const uint2 c = p.cand[base + i];
        if (c.y != 0xFFFFFFFFu) f(c.x, seg, c.y, base + i);
      }
    }
  };

  // ---- sweep 1: accept() (tombstones / filter), the accepted count, AND / OR of every key word ----
  {
    uint32_t t_and[NW], t_or[NW];
#pragma unroll
    for (uint32_t w = 0; w < NW; w++) {
      t_and[w] = 0xFFFFFFFFu;
      t_or[w] = 0u;
    }
    uint32_t nv = 0;
    for_each([&](uint32_t a, uint32_t seg, uint32_t doc, uint64_t at) {
      const uint32_t *del = flt ? p.reject_table[(size_t)(flt - 1) * p.n_segs + seg] : p.segs[seg].deleted;
      if (del && ((del[doc >> 5] >> (doc & 31)) & 1u)) {
        p.cand[at].y = 0xFFFFFFFFu;
        return;
      }
      uint32_t K[NW];
      sorted_key(p, a, seg, doc, K);
      if constexpr (CURSOR) {
        if (cur_on) {
          int c = 0;
#pragma unroll
          for (uint32_t w = 0; w < NW; w++) {
            const uint32_t y = s_cur[1 + w];
            if (c == 0) c = K[w] < y ? -1 : (K[w] > y ? 1 : 0);
          }
          if (c <= 0) {  // on an earlier page
            if (c == 0) sh_seen = 1u;
            p.cand[at].y = 0xFFFFFFFFu;
            return;
          }
        }
      }
#pragma unroll
      for (uint32_t w = 0; w < NW; w++) {
        t_and[w] &= K[w];
        t_or[w] |= K[w];
      }
      nv++;
    });
#pragma unroll
    for (uint32_t w = 0; w < NW; w++) {
      uint32_t x = t_and[w], y = t_or[w];
      for (int o = 32; o > 0; o >>= 1) {
        x &= __shfl_xor(x, o, 64);
        y |= __shfl_xor(y, o, 64);
      }
      if (lane == 0) {
        atomicAnd(&s_and[w], x);
        atomicOr(&s_or[w], y);
      }
    }
    nv = wave_sum(nv);
    if (lane == 0) atomicAdd(&sh_nvalid, nv);
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t n = 0;
    for (uint32_t w = 0; w < NW; w++) s_slot[w] = s_and[w] != s_or[w] ? n++ : 0xFFFFFFFFu;
    sh_nvary = n;
    if (p.out_matched) p.out_matched[q] = sh_nvalid;
  }
  __syncthreads();
  const uint32_t nvalid = sh_nvalid, nvary = sh_nvary;
  const uint32_t nout = nvalid < k ? nvalid : k;

  uint32_t k_done = 0;
  bool have_prev = false;
  while (k_done < nout) {
    const uint32_t target = nout - k_done > CAP ? k_done + CAP : nout;
    const bool last = target == nout;
    const uint32_t cap_last = last_range_cap(nout - k_done, CAP);
    const bool all = last && nvalid - k_done <= cap_last;  // everything left fits: no select
    __syncthreads();
    if (tid < NW) s_pre[tid] = s_dm[tid] = 0u;
    if (tid == 0) {
      sh_need = target;
      sh_done = all ? 1u : 0u;
      sh_taken = all ? nvalid : 0u;
      sh_nwin = 0;
    }
    __syncthreads();
    if (!all) {
      for (uint32_t lev = 0; lev < NW * 4; lev++) {
        const uint32_t wd = lev >> 2, shift = 24u - 8u * (lev & 3u), bm = 0xFFu << shift;
        if (((s_and[wd] ^ s_or[wd]) & bm) == 0u) continue;  // the same byte in every key (uniform)
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for_each([&](uint32_t a, uint32_t seg, uint32_t doc, uint64_t) {
          uint32_t K[NW];
          sorted_key(p, a, seg, doc, K);
          if (sorted_cmp(K, s_pre, s_dm) != 0) return;
          uint32_t wv = 0;
#pragma unroll
          for (uint32_t w = 0; w < NW; w++) wv = w == wd ? K[w] : wv;
          hist_add_by_bin(hist, (wv >> shift) & 255u, lane);  // (ties are the normal case here)
        });
        __syncthreads();
        if (wave == 0) {  // lane l owns bins 4l .. 4l+3 (ascending; the twin of select_topk_kernel's pick)
          const uint32_t b0 = 4u * lane;
          const uint32_t h0 = hist[b0], h1 = hist[b0 + 1], h2 = hist[b0 + 2], h3 = hist[b0 + 3];
          const uint32_t tot = h0 + h1 + h2 + h3;
          uint32_t incl = tot;
          for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(incl, o, 64);
            if ((int)lane >= o) incl += v;
          }
          const uint32_t need = sh_need, excl = incl - tot;
          if (excl < need && need <= incl) {  // exactly one lane
            uint32_t cum = excl, b = b0, h = h0;
            if (cum + h < need) { cum += h; b = b0 + 1; h = h1; }
            if (cum + h < need) { cum += h; b = b0 + 2; h = h2; }
            if (cum + h < need) { cum += h; b = b0 + 3; h = h3; }
            s_pre[wd] |= b << shift;
            s_dm[wd] |= bm;
            sh_need = need - cum;                                 // rank of the target key inside the bucket
            const uint32_t taken = (target - (need - cum)) + h;  // keys with prefix <= the chosen one
            sh_taken = taken;
            sh_done = (h == need - cum || (last && taken - k_done <= cap_last)) ? 1u : 0u;
          }
        }
        __syncthreads();
        if (sh_done) break;
      }
    }
    const uint32_t taken = sh_taken;
    const uint32_t count = (taken - k_done) < CAP ? (taken - k_done) : CAP;
    // ---- gather the varying words of this range's keys ----
    for_each([&](uint32_t a, uint32_t seg, uint32_t doc, uint64_t) {
      uint32_t K[NW];
      sorted_key(p, a, seg, doc, K);
      bool win = all || sorted_cmp(K, s_pre, s_dm) <= 0;
      if (win && have_prev) win = sorted_cmp(K, s_qpre, s_qdm) > 0;
      const uint32_t at = wave_compact_slot(&sh_nwin, win, lane);
      if (win && at < CAP) {
#pragma unroll
        for (uint32_t w = 0; w < NW; w++)
          if (s_slot[w] != 0xFFFFFFFFu) w_key[s_slot[w] * CAP + at] = K[w];
      }
    });
    __syncthreads();
    // ---- bitonic sort of the entries' indices, ascending key (indices >= count: padding, last) ----
    uint32_t n2 = 1;
    while (n2 < count) n2 <<= 1;
    for (uint32_t i = tid; i < n2; i += NT) w_idx[i] = (uint16_t)i;
    __syncthreads();
    auto less = [&](const uint32_t x, const uint32_t y) {
      if (x >= count || y >= count) return x < count ? true : (y < count ? false : x < y);
      for (uint32_t r = 0; r < nvary; r++) {
        const uint32_t u = w_key[r * CAP + x], v = w_key[r * CAP + y];
        if (u != v) return u < v;
      }
      return false;
    };
    for (uint32_t size = 2; size <= n2; size <<= 1) {
      for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
        for (uint32_t t = tid; t < (n2 >> 1); t += NT) {
          const uint32_t i = 2 * t - (t & (stride - 1));  // lower index of the pair
          const uint32_t j = i + stride;
          const bool up = (i & size) == 0;
          const uint32_t xi = w_idx[i], xj = w_idx[j];
          if (up ? less(xj, xi) : less(xi, xj)) {
            w_idx[i] = (uint16_t)xj;
            w_idx[j] = (uint16_t)xi;
          }
        }
        __syncthreads();
      }
    }
    // ---- write the range (the final one drops what it took beyond k) ----
    const uint32_t emit = target - k_done;
    for (uint32_t i = tid; i < emit; i += NT) {
      const uint32_t e = w_idx[i];
      auto word = [&](const uint32_t w) { return s_slot[w] != 0xFFFFFFFFu ? w_key[s_slot[w] * CAP + e] : s_and[w]; };
      float score = 0.0f;  // (MatchOnly: no `_score` part, the hit's score is 0.0, query/wand.rs match_only_loop)
      if (p.score_parts) {
        const uint32_t sp = (uint32_t)__builtin_ctz(p.score_parts);
        const uint32_t a = word(3 * sp + 2) ^ (((p.desc_parts >> sp) & 1u) ? 0xFFFFFFFFu : 0u);
        score = key_to_float((int32_t)(a ^ 0x80000000u));
      }
      p.out_doc[(size_t)q * k + k_done + i] = word(NW - 1);
      p.out_seg[(size_t)q * k + k_done + i] = word(NW - 2);
      p.out_score[(size_t)q * k + k_done + i] = score;
    }
    if (tid < NW) {
      s_qpre[tid] = s_pre[tid];
      s_qdm[tid] = s_dm[tid];
    }
    k_done = target;
    have_prev = true;
  }
  zero_rows(p.out_doc, p.out_seg, p.out_score, q, k, nout, tid, NT);
  if (tid == 0) p.out_count[q] = nout;
  if constexpr (CURSOR) {
    if (tid == 0) p.out_seen[q] = cur_on ? sh_seen : 1u;
  }
}

}  // namespace slg
