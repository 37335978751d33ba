// slg_tophits.hpp — the top_hits aggregation (slg_batch_prepare_top_hits; TopHitsCollector and merge_top_hits,
// query/aggs/mod.rs:1870-1981, :2426-2459): per list — the root, or every bucket of a root bucket node — the
// from + size <= 64 best matched docs under the node's SortKey (parts, a Missing value after every value in both
// orders, then segment, then doc: query/sort.rs:80-123), of which the rows [from, from + size) are reported.
//
// One workgroup of 256 threads per query, behind agg_kernel (which wrote the parent's count row), over the
// candidate region the batch's scoring kernel left.  A candidate's score is its cand.x; in a batch whose
// ScoreMode is MatchOnly (a field sort without a `_score` part) it is 0.0, as the batch's rows report it.
//   one list    (a root node, a child of a filter node): every wave walks its slices converged and keeps its own
//               best L = from + size sorted one per lane — the list's last is broadcast, a ballot finds the
//               candidates that beat it, each is inserted by shfl_up from its ballot position — the four lists
//               meet in LDS and wave 0 merges them
//   many lists  (a child of a terms, histogram, range or date_histogram root): the workgroup prefix-sums the
//               parent's count row into one cursor per list (its run's first slot), a second walk calls agg_buckets
//               on the parent and takes a slot of the bucket's run with one atomicAdd on its cursor (8-byte
//               entries: slice, position in the slice), and after a barrier a wave per list reads its run 64
//               entries at a time and keeps the best L in lanes, as above.  Nodes under one parent that follow one
//               another in the spec share the runs; a query holds the runs of one parent at a time, so a node whose
//               parent differs from the many-lists node before it builds them again.
//               A cursor ends at its run's end, so the run of a list is [cursor - count, cursor).
// The slot an entry lands in depends on scheduling; the lists do not, because the key is a total order.  Every
// output element is written on every run (zeros past the counts; all zeros for a query whose runs do not fit
// max_entries: status 1), so a rerun needs no memset.  No compare-and-swap loop.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_aggs.hpp"
#include "slg_wave.hpp"

namespace slg {

constexpr uint32_t kTopHitsThreads = kAggThreads;
constexpr uint32_t kTopHitsMaxNodes = 4;    // SLG_MAX_TOP_HITS_NODES
constexpr uint32_t kTopHitsMaxList = 64;    // SLG_MAX_TOP_HITS: one entry per lane
constexpr uint32_t kTopHitsEntryWords = kSortWords + 1;  // of a kept entry: the key, then the ordered score
constexpr uint32_t kTopHitsMergeWords = (kTopHitsThreads / 64) * 64 * kTopHitsEntryWords;  // the four waves' lists
constexpr uint32_t kTopHitsLdsLists = 4096;  // parents of up to this many rows keep their cursors in LDS

struct TopHitsNodeDev {
  int32_t parent;  // -1: the root; else a root bucket node of the aggregation spec
  uint32_t from, size;
  uint32_t lists;     // 1, or the parent's rows
  uint32_t list_off;  // first list in the query's count array
  uint32_t hit_off;   // first cell in the query's hit arrays
  uint32_t n_parts, score_parts, desc_parts;  // the node's sort (as SortedSelectParams)
  uint32_t many;      // the many-lists path
  uint32_t first;     // the node builds its parent's runs: the many-lists node before it has another parent (or there
                      // is none); a node with first = 0 reads the runs the one before it left
  uint32_t pad;
};

struct TopHitsParams {
  const QueryRef *queries;
  const uint32_t *slice_seg;
  const uint64_t *slice_cbeg;
  const uint32_t *slice_ccnt;
  const uint2 *cand;  // .x ordered score, .y doc (0xFFFFFFFF: dropped)
  const SegDev *segs;
  const uint32_t *q_filter;
  const uint32_t *const *reject_table;
  const AggNodeDev *nodes;  // the aggregation spec's nodes and columns (null without one)
  const ColumnDev *cols;
  uint32_t n_segs, nq;
  uint32_t count_cells;
  const uint32_t *counts;             // [nq * count_cells] agg_kernel's count tables
  const TopHitsNodeDev *th;           // [n_th]
  const SortColDev *sort_cols;        // [n_th][kSortMaxParts * n_segs]
  uint32_t n_th;
  uint32_t match_only;                // the batch's rows carry 0.0 as their score
  uint32_t max_entries;               // run slots of one query
  uint32_t cursor_words;              // of one query's slice of `cursors` (0: every parent's cursors fit LDS)
  uint2 *entries;                     // [nq * max_entries]
  uint32_t *cursors;                  // [nq * cursor_words]
  uint32_t hit_cells, list_cells;     // of one query
  uint32_t *out;                      // doc, seg, score [nq * hit_cells] each, count [nq * list_cells], status [nq] ...
  const uint32_t *flag;               // ... and behind them the index's error word as the batch's last kernel left it
  unsigned long long *out_matched;    // [nq] accepted docs, or null (the select or agg_kernel wrote them)
};

// the first word of output array i (0 doc, 1 seg, 2 score, 3 count, 4 status, 5 the error word)
__host__ __device__ inline size_t top_hits_out(uint32_t i, uint32_t nq, uint32_t hit_cells, uint32_t list_cells) {
  const size_t h = (size_t)nq * hit_cells, l = (size_t)nq * list_cells;
  return i < 4u ? (size_t)i * h : 3u * h + l + (i - 4u) * (size_t)nq;
}

// the sort of one node, in the shape sorted_key reads
struct TopHitsSort {
  const SortColDev *sort_cols;
  uint32_t n_segs, n_parts, score_parts, desc_parts;
};

// x < y, word by word
__device__ __forceinline__ bool top_hits_less(const uint32_t (&x)[kSortWords], const uint32_t (&y)[kSortWords]) {
  int c = 0;
#pragma unroll
  for (uint32_t w = 0; w < kSortWords; w++)
    if (c == 0) c = x[w] < y[w] ? -1 : (x[w] > y[w] ? 1 : 0);
  return c < 0;
}

// The best L entries seen so far, sorted, lane l holding the l-th (all-ones key: none; no doc's key is all-ones,
// its first word is 0 or 1).  offer: one candidate per lane (`has`), all lanes of the wave together.
struct TopHitsList {
  uint32_t K[kSortWords], a;
  __device__ __forceinline__ void init() {
#pragma unroll
    for (uint32_t w = 0; w < kSortWords; w++) K[w] = 0xFFFFFFFFu;
    a = 0u;
  }
  __device__ __forceinline__ bool real() const { return K[0] != 0xFFFFFFFFu; }
  __device__ __forceinline__ void offer(const bool has, const uint32_t (&C)[kSortWords], const uint32_t ca,
                                        const uint32_t L, const uint32_t lane) {
    uint32_t W[kSortWords];
#pragma unroll
    for (uint32_t w = 0; w < kSortWords; w++) W[w] = (uint32_t)__shfl((int)K[w], (int)(L - 1u), 64);
    // (the list's last as it is now: it only gets better, so a candidate that does not beat it never enters)
    uint64_t todo = __ballot(has && top_hits_less(C, W));
    while (todo) {
      const uint32_t c = (uint32_t)__builtin_ctzll(todo);
      todo &= todo - 1ull;
      uint32_t B[kSortWords];
#pragma unroll
      for (uint32_t w = 0; w < kSortWords; w++) B[w] = (uint32_t)__shfl((int)C[w], (int)c, 64);
      const uint32_t ba = (uint32_t)__shfl((int)ca, (int)c, 64);
      const uint64_t after = __ballot(top_hits_less(B, K));  // the lanes whose entry comes after this one
      if (after == 0ull) continue;
      const uint32_t ins = (uint32_t)__builtin_ctzll(after);
#pragma unroll
      for (uint32_t w = 0; w < kSortWords; w++) {
        const uint32_t up = (uint32_t)__shfl_up((int)K[w], 1, 64);
        K[w] = lane > ins ? up : (lane == ins ? B[w] : K[w]);
      }
      const uint32_t upa = (uint32_t)__shfl_up((int)a, 1, 64);
      a = lane > ins ? upa : (lane == ins ? ba : a);
      if (ins < L && todo) {  // the last got better: the candidates that no longer beat it leave the queue
#pragma unroll
        for (uint32_t w = 0; w < kSortWords; w++) W[w] = (uint32_t)__shfl((int)K[w], (int)(L - 1u), 64);
        todo &= __ballot(top_hits_less(C, W));
      }
    }
  }
};

// The candidates of query qr as agg_walk<true> walks them — a wave per slice, a lane per candidate, f for ALL
// lanes of the wave together — with what a hit needs beyond (seg, doc): the candidate's ordered score, its slice
// and its position in the slice.  ok false: no candidate, a dropped one, a tombstone or a doc the filter rejects.
template <typename F>
__device__ __forceinline__ void top_hits_walk(const TopHitsParams &p, const QueryRef &qr, const uint32_t flt,
                                              const uint32_t wave, const uint32_t lane, F &&f) {
  for (uint32_t s = qr.slice_begin + wave; s < qr.slice_end; s += kTopHitsThreads / 64) {
    const uint64_t base = p.slice_cbeg[s];
    const uint32_t n = p.slice_ccnt[s];
    const uint32_t seg = p.slice_seg[s];
    const uint32_t *del = flt ? p.reject_table[(size_t)(flt - 1) * p.n_segs + seg] : p.segs[seg].deleted;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
      const uint32_t i = i0 + lane;
      uint2 c = make_uint2(0u, 0xFFFFFFFFu);
      if (i < n) c = p.cand[base + i];
      const bool ok = c.y != 0xFFFFFFFFu && !(del && ((del[c.y >> 5] >> (c.y & 31)) & 1u));
      f(ok, seg, c.y, c.x, s, i);
    }
  }
}

template <bool EXT>
static __global__ void __launch_bounds__(kTopHitsThreads) top_hits_kernel(TopHitsParams p) {
  extern __shared__ uint32_t th_lds[];  // the four waves' lists, then the cursors of a parent that fits
  __shared__ uint32_t sh_wtot[kTopHitsThreads / 64], sh_sum, sh_fail;
  __shared__ unsigned long long sh_tot;
  constexpr uint32_t NT = kTopHitsThreads, NW = kSortWords, EW = kTopHitsEntryWords;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t q = blockIdx.x;
  if (q >= p.nq) return;
  const QueryRef qr = p.queries[q];
  const uint32_t flt = p.q_filter ? p.q_filter[q] : 0u;
  const uint32_t zero_a = ordered_score(0.0f);
  uint32_t *const out_doc = p.out + top_hits_out(0, p.nq, p.hit_cells, p.list_cells) + (size_t)q * p.hit_cells;
  uint32_t *const out_seg = p.out + top_hits_out(1, p.nq, p.hit_cells, p.list_cells) + (size_t)q * p.hit_cells;
  uint32_t *const out_score = p.out + top_hits_out(2, p.nq, p.hit_cells, p.list_cells) + (size_t)q * p.hit_cells;
  uint32_t *const out_count = p.out + top_hits_out(3, p.nq, p.hit_cells, p.list_cells) + (size_t)q * p.list_cells;
  uint32_t *const out_status = p.out + top_hits_out(4, p.nq, p.hit_cells, p.list_cells);
  if (q == 0 && tid == 0) p.out[top_hits_out(5, p.nq, p.hit_cells, p.list_cells)] = *p.flag;
  const uint32_t *const qcounts = p.counts + (size_t)q * p.count_cells;
  uint2 *const entries = p.entries + (size_t)q * p.max_entries;
  uint32_t *const s_merge = th_lds;
  uint32_t *const s_cursor = th_lds + kTopHitsMergeWords;
  if (tid == 0) {
    sh_sum = 0u;
    sh_fail = 0u;
    sh_tot = 0ull;
  }
  __syncthreads();

  if (p.out_matched) {  // (a batch in score order without an aggregation spec: nobody else counts)
    uint32_t nv = 0;
    top_hits_walk(p, qr, flt, wave, lane, [&](const bool ok, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {
      nv += ok ? 1u : 0u;
    });
    nv = wave_sum(nv);
    if (lane == 0 && nv) atomicAdd(&sh_sum, nv);
    __syncthreads();
    if (tid == 0) {
      p.out_matched[q] = sh_sum;
      sh_sum = 0u;
    }
    __syncthreads();
  }

  // ---- do the runs of every parent fit?  (the sum of a parent's count row: what the fill will store) ----
  for (uint32_t t = 0; t < p.n_th; t++) {
    const TopHitsNodeDev &th = p.th[t];
    if (!th.many || !th.first) continue;
    const uint32_t *row = qcounts + p.nodes[th.parent].off;
    unsigned long long sum = 0ull;  // (64 bits: a doc with several values is in several lists)
    for (uint32_t l = tid; l < th.lists; l += NT) sum += agg_read_back<true>(row + l);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0 && sum) atomicAdd(&sh_tot, sum);
    __syncthreads();
    if (tid == 0) {
      if (sh_tot > (unsigned long long)p.max_entries) sh_fail = 1u;
      sh_tot = 0ull;
    }
    __syncthreads();
  }
  if (sh_fail) {  // (workgroup-uniform) the caller takes this query to the CPU path
    for (uint32_t i = tid; i < p.hit_cells; i += NT) {
      out_doc[i] = 0u;
      out_seg[i] = 0u;
      out_score[i] = 0u;
    }
    for (uint32_t i = tid; i < p.list_cells; i += NT) out_count[i] = 0u;
    if (tid == 0) out_status[q] = 1u;
    return;
  }
  if (tid == 0) out_status[q] = 0u;

  // the cells of one list from the wave's finished list: lanes [from, L) hold them
  auto write_list = [&](const TopHitsNodeDev &th, const uint32_t list, const TopHitsList &best) {
    const uint32_t L = th.from + th.size;
    const uint32_t held = (uint32_t)__popcll(__ballot(best.real() && lane < L));
    const uint32_t left = held > th.from ? held - th.from : 0u;
    const uint32_t cnt = left < th.size ? left : th.size;
    if (lane >= th.from && lane < L) {
      const uint32_t j = lane - th.from;
      const bool have = j < cnt;
      const size_t o = (size_t)th.hit_off + (size_t)list * th.size + j;
      out_doc[o] = have ? best.K[NW - 1] : 0u;
      out_seg[o] = have ? best.K[NW - 2] : 0u;
      out_score[o] = have ? __float_as_uint(key_to_float((int32_t)(best.a ^ 0x80000000u))) : 0u;
    }
    if (lane == 0) out_count[th.list_off + list] = cnt;
  };

  for (uint32_t t = 0; t < p.n_th; t++) {
    const TopHitsNodeDev th = p.th[t];
    const uint32_t L = th.from + th.size;
    const TopHitsSort sort{p.sort_cols + (size_t)t * kSortMaxParts * p.n_segs, p.n_segs, th.n_parts, th.score_parts,
                           th.desc_parts};
    if (!th.many) {
      // ---- one list: a list per wave, merged by wave 0 ----
      TopHitsList best;
      best.init();
      top_hits_walk(p, qr, flt, wave, lane,
                    [&](bool ok, const uint32_t seg, const uint32_t doc, const uint32_t x, uint32_t, uint32_t) {
                      if (EXT && th.parent >= 0) ok = ok && agg_filter_passes(p, p.nodes[th.parent], seg, doc);
                      const uint32_t ca = p.match_only ? zero_a : x;
                      uint32_t C[NW];
#pragma unroll
                      for (uint32_t w = 0; w < NW; w++) C[w] = 0xFFFFFFFFu;
                      if (ok) sorted_key(sort, ca, seg, doc, C);
                      best.offer(ok, C, ca, L, lane);
                    });
      __syncthreads();  // (the region is the previous node's)
      {
        uint32_t *e = s_merge + ((size_t)wave * 64u + lane) * EW;
#pragma unroll
        for (uint32_t w = 0; w < NW; w++) e[w] = best.K[w];
        e[NW] = best.a;
      }
      __syncthreads();
      if (wave == 0) {
        for (uint32_t w2 = 1; w2 < NT / 64u; w2++) {
          const uint32_t *e = s_merge + ((size_t)w2 * 64u + lane) * EW;
          uint32_t C[NW];
#pragma unroll
          for (uint32_t w = 0; w < NW; w++) C[w] = e[w];
          best.offer(C[0] != 0xFFFFFFFFu && lane < L, C, e[NW], L, lane);
        }
        write_list(th, 0u, best);
      }
      continue;
    }

    // ---- many lists ----
    const AggNodeDev &par = p.nodes[th.parent];
    const uint32_t *const row = qcounts + par.off;
    const bool lds_cur = th.lists <= kTopHitsLdsLists;
    uint32_t *const cursor = lds_cur ? s_cursor : p.cursors + (size_t)q * p.cursor_words;
    if (th.first) {
      // offsets: consecutive lists per thread, a scan of the 256 partial sums; cursor[l] = the first slot of run l
      __syncthreads();  // (the cursors are the previous parent's)
      const uint32_t per = (th.lists + NT - 1u) / NT;
      const uint32_t l0 = tid * per;
      uint32_t sum = 0;
      for (uint32_t j = 0; j < per; j++) sum += l0 + j < th.lists ? agg_read_back<true>(row + l0 + j) : 0u;
      const uint32_t ex = wave_excl_scan(sum, lane);
      if (lane == 63u) sh_wtot[wave] = ex + sum;
      __syncthreads();
      uint32_t run = ex;
      for (uint32_t w = 0; w < wave; w++) run += sh_wtot[w];
      for (uint32_t j = 0; j < per && l0 + j < th.lists; j++) {
        cursor[l0 + j] = run;
        run += agg_read_back<true>(row + l0 + j);
      }
      __syncthreads();
      // fill: every bucket the doc was counted in takes the next slot of its run
      top_hits_walk(p, qr, flt, wave, lane,
                    [&](const bool ok, const uint32_t seg, const uint32_t doc, uint32_t, const uint32_t s,
                        const uint32_t i) {
                      if (!ok) return;
                      agg_buckets<EXT>(p, par, seg, doc, [&](const uint32_t b) {
                        if (b >= th.lists) return;
                        const uint32_t slot = atomicAdd(&cursor[b], 1u);
                        if (slot < p.max_entries) entries[slot] = make_uint2(s, i);  // (the sum was checked: a guard)
                      });
                    });
      __syncthreads();
    }
    // select: a wave per list; its run is [cursor - count, cursor)
    for (uint32_t l = wave; l < th.lists; l += NT / 64u) {
      const uint32_t n = agg_read_back<true>(row + l);
      uint32_t en = 0;
      if (n) en = lds_cur ? cursor[l] : agg_read_back<true>(cursor + l);
      en = en < p.max_entries ? en : p.max_entries;
      const uint32_t st = en > n ? en - n : 0u;
      TopHitsList best;
      best.init();
      for (uint32_t base = st; base < en; base += 64u) {
        const uint32_t pos = base + lane;
        bool has = pos < en;
        uint32_t C[NW], ca = 0u;
#pragma unroll
        for (uint32_t w = 0; w < NW; w++) C[w] = 0xFFFFFFFFu;
        unsigned long long e = 0ull;
        if (has)
          e = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(entries + pos), __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);  // (another wave's store: read past the L1)
        const uint32_t s = (uint32_t)e, i = (uint32_t)(e >> 32);
        // (an entry is a slice of this query and a position in it: a guard, not a path)
        has = has && s >= qr.slice_begin && s < qr.slice_end && i < p.slice_ccnt[s < qr.slice_end ? s : qr.slice_begin];
        uint2 c = make_uint2(0u, 0xFFFFFFFFu);
        if (has) c = p.cand[p.slice_cbeg[s] + i];
        has = has && c.y != 0xFFFFFFFFu;
        if (has) {
          ca = p.match_only ? zero_a : c.x;
          sorted_key(sort, ca, p.slice_seg[s], c.y, C);
        }
        best.offer(has, C, ca, L, lane);
      }
      write_list(th, l, best);
    }
  }
}

}  // namespace slg
