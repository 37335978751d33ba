// slg_collapse.hpp — field collapsing (SearchRequest::collapse): one hit per group, inner hits.
//
// Semantics restated from api/reader.rs:3499-3562 (collapse_hits) and :3578-3595 (collapse_value); the rows of
// a query are the reference's hits in SortKey order.  A row without a value of the column is dropped, a row
// with more than one fails the query (status 1), every other row joins the group of its ordinal; groups are
// ordered by first appearance and a group's first row is its representative (the stable sort at :3532 sorts
// rows that are in key order already).  Inner hits are the other rows of the group: in row order, or — with an
// inner sort that differs from the batch's — by the full sort key (parts, then segment, doc), and of those the
// rows [from, from + size).  The outputs in full: include/searchlite_gpu.h (slg_batch_prepare_collapse).
//
// Shape: one workgroup of 256 threads per query, everything in LDS, sized at launch from k: 12 bytes per row of
// the power of two >= max(k, 64) (48 KB at k = 4096: three workgroups per CU).  A query works on pn = the power
// of two >= its own n rows, so a short query in a wide batch sorts and probes little.
//   1. every row gathers its ordinal from the column's CSR into ord[i]; a multi-valued row raises the status
//   2. an open-addressing table of 2 pn slots of ROW indices, a slot's key being ord[its row]: an empty slot is
//      claimed with atomicCAS, a slot of the same ordinal takes atomicMin(row), anything else probes on.  A
//      slot's key never changes once set, so probing stays consistent whatever the order of the threads, and
//      each group's slot ends at its smallest row: the representative
//   3. an exclusive scan of `is representative` in row order numbers the groups by first appearance
//   4. (group << 12 | row) of every row with a value, bitonic-sorted over the table's first half: each group
//      is a run in row order with its representative first; the run starts give the sizes
//   5. inner hits in row order are slices of the runs; under an inner sort one wave per reported group keeps
//      the best from + size <= 64 members sorted one per lane (a member's key: sorted_key's words),
//      reading the run 64 members at a time and inserting those that beat the list's last by ballot + shuffle
// Nothing depends on scheduling: the table's final content, the scan, the sort of distinct keys and the
// per-wave insertion are all functions of the rows.  Every element of every side array is written on every
// run (zeros past the counts), so a rerun needs no memset.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_wave.hpp"

namespace slg {

constexpr uint32_t kCollapseThreads = 256;
constexpr uint32_t kCollapseMaxRows = 4096;  // SLG_MAX_COLLAPSE_ROWS
constexpr uint32_t kCollapseRowBits = 12;    // a row index in the sort key
constexpr uint32_t kCollapseRowsPerThread = kCollapseMaxRows / kCollapseThreads;
constexpr uint32_t kCollapseNone = 0xFFFFFFFFu;  // a row without a value; an empty slot; a pad key
constexpr uint32_t kCollapseMisc = 16;           // words behind the arrays: status, valid rows, wave sums
static_assert((1u << kCollapseRowBits) == kCollapseMaxRows, "row bits of the sort key");

struct CollapseParams {
  const ColumnDev *cols;        // [n_segs] the keyword column (vals nullptr: no doc of the segment has a value)
  const SortColDev *sort_cols;  // [kSortMaxParts * n_segs] the inner sort: part p of segment s at p * n_segs + s
  uint32_t n_segs;
  uint32_t n_parts;  // of the inner sort; 0: members stay in row order
  uint32_t score_parts, desc_parts;  // bit p: part p is `_score` / descends (as SortedSelectParams)
  const uint32_t *out_doc, *out_seg;  // the batch's rows [nq * k]: read only
  const float *out_score;
  const uint32_t *out_count;  // [nq]
  uint32_t nq, k;
  uint32_t groups, from, size;  // group_limit, inner_from, inner_size
  uint32_t lds_rows;            // rows the LDS arrays hold: a power of two >= k
  uint32_t *side;               // the arrays of slg_batch_fetch_collapse, back to back (collapse_side) ...
  const uint32_t *flag;         // ... and behind them the index's error word as the batch's last kernel left it
};

// The side arrays in the argument order of slg_batch_fetch_collapse — 0 n_groups, 1 total_groups, 2 status [nq];
// 3 group_row, 4 group_ord, 5 group_size, 6 group_doc, 7 group_seg, 8 group_score, 9 inner_count [nq * groups];
// 10 inner_row, 11 inner_doc, 12 inner_seg, 13 inner_score [nq * groups * size]: the first word of array i
// (i = 14: the words of all)
enum : uint32_t {
  kClNGroups = 0, kClTotal, kClStatus, kClRow, kClOrd, kClSize, kClDoc, kClSeg, kClScore, kClInnerCount,
  kClInnerRow, kClInnerDoc, kClInnerSeg, kClInnerScore, kClArrays
};
__host__ __device__ inline size_t collapse_side(uint32_t i, uint32_t nq, uint32_t groups, uint32_t size) {
  const size_t per_g = (size_t)nq * groups, per_i = per_g * size;
  if (i < 3u) return (size_t)i * nq;
  if (i < 10u) return 3u * (size_t)nq + (i - 3u) * per_g;
  return 3u * (size_t)nq + 7u * per_g + (i - 10u) * per_i;
}

inline uint32_t collapse_lds_rows(uint32_t k) {
  uint32_t r = 64;
  while (r < k) r <<= 1;
  return r;
}
inline size_t collapse_lds_bytes(uint32_t lds_rows) { return ((size_t)lds_rows * 3 + kCollapseMisc) * 4; }

// x < y, word by word
__device__ __forceinline__ bool collapse_less(const uint32_t (&x)[kSortWords], const uint32_t (&y)[kSortWords]) {
  int c = 0;
#pragma unroll
  for (uint32_t w = 0; w < kSortWords; w++)
    if (c == 0) c = x[w] < y[w] ? -1 : (x[w] > y[w] ? 1 : 0);
  return c < 0;
}

static __global__ void __launch_bounds__(kCollapseThreads) collapse_kernel(CollapseParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr uint32_t NT = kCollapseThreads, NONE = kCollapseNone, RB = kCollapseRowBits;
  constexpr uint32_t RMASK = (1u << RB) - 1u;
  uint32_t *const s_ord = reinterpret_cast<uint32_t *>(smem);  // [lds_rows] a row's ordinal
  uint32_t *const s_tab = s_ord + p.lds_rows;   // [2 * lds_rows] the table; then the sort keys and run starts
  uint32_t *const s_misc = s_tab + 2u * p.lds_rows;  // [0] status, [1] rows with a value, [2 .. 5] wave sums
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t q = blockIdx.x;
  if (q >= p.nq) return;
  const uint32_t k = p.k, G = p.groups, S = p.size, from = p.from;
  const uint32_t *const odoc = p.out_doc + (size_t)q * k;
  const uint32_t *const oseg = p.out_seg + (size_t)q * k;
  const float *const oscore = p.out_score + (size_t)q * k;
  auto side = [&](const uint32_t i) { return p.side + collapse_side(i, p.nq, G, S); };
  if (q == 0 && tid == 0) *side(kClArrays) = *p.flag;  // (one copy fetches the arrays and the word)
  uint32_t n = p.out_count[q];
  n = n < k ? n : k;
  n = n < p.lds_rows ? n : p.lds_rows;  // (the host sized the arrays for k: a guard, not a path)
  uint32_t pn = 2;
  while (pn < n) pn <<= 1;  // <= lds_rows, a power of two itself
  const uint32_t tbits = 32u - (uint32_t)__clz((int)pn);  // log2 of the table's 2 pn slots
  const uint32_t tmask = 2u * pn - 1u;
  uint32_t *const s_key = s_tab;         // [pn] (steps 4, 5)
  uint32_t *const s_start = s_tab + pn;  // [pn] first position of each group's run

  // ---- 1. ordinals ----
  if (tid < kCollapseMisc) s_misc[tid] = 0u;
  for (uint32_t i = tid; i < 2u * pn; i += NT) s_tab[i] = NONE;
  __syncthreads();
  {
    bool multi = false;
    for (uint32_t i = tid; i < n; i += NT) {
      const uint32_t seg = oseg[i], doc = odoc[i];
      uint32_t o = NONE;
      if (seg < p.n_segs) {
        const ColumnDev col = p.cols[seg];
        if (col.vals) {
          uint32_t a, e;
          column_range(col, doc, a, e);
          if (e - a == 1u) o = col.ords()[a];
          multi = multi || (e > a && e - a > 1u);
        }
      }
      s_ord[i] = o;
    }
    if (multi) atomicOr(&s_misc[0], 1u);
  }
  __syncthreads();
  const uint32_t failed = s_misc[0];
  uint32_t total = 0, m = 0;

  if (!failed) {
    // ---- 2. the table: a group's slot ends at its smallest row ----
    for (uint32_t i = tid; i < n; i += NT) {
      const uint32_t o = s_ord[i];
      if (o == NONE) continue;
      uint32_t h = (o * 0x9E3779B1u) >> (32u - tbits);
      for (uint32_t probes = 0; probes <= tmask; probes++) {  // (2 pn slots, at most pn keys: it ends long before)
        uint32_t cur = __atomic_load_n(&s_tab[h], __ATOMIC_RELAXED);
        if (cur == NONE) {
          cur = atomicCAS(&s_tab[h], NONE, i);
          if (cur == NONE) break;
        }
        if (s_ord[cur] == o) {  // (whichever row of the group holds the slot: its key is o for good)
          atomicMin(&s_tab[h], i);
          break;
        }
        h = (h + 1u) & tmask;
      }
    }
    __syncthreads();

    // ---- 3. groups numbered by first appearance: a thread owns `per` consecutive rows ----
    const uint32_t per = pn >= NT ? pn / NT : 1u;
    uint32_t slot[kCollapseRowsPerThread];  // the slot of each of this thread's rows, then its sort key
    uint32_t reps = 0, n_reps = 0, n_valid = 0;
#pragma unroll
    for (uint32_t r = 0; r < kCollapseRowsPerThread; r++) {
      slot[r] = NONE;
      const uint32_t i = tid * per + r;
      if (r < per && i < n) {
        const uint32_t o = s_ord[i];
        if (o != NONE) {
          uint32_t h = (o * 0x9E3779B1u) >> (32u - tbits);
          // (the row's group is in the table: no empty slot lies before it)
          for (uint32_t probes = 0; probes < tmask && s_ord[s_tab[h] & (p.lds_rows - 1u)] != o; probes++) h = (h + 1u) & tmask;
          slot[r] = h;
          n_valid++;
          if (s_tab[h] == i) {
            reps |= 1u << r;
            n_reps++;
          }
        }
      }
    }
    const uint32_t in_wave = wave_excl_scan(n_reps, lane);
    if (lane == 63u) s_misc[2 + wave] = in_wave + n_reps;
    if (n_valid) atomicAdd(&s_misc[1], n_valid);
    __syncthreads();  // (every lookup is done: the slots may change their meaning)
    uint32_t g_next = in_wave;
    for (uint32_t w = 0; w < NT / 64u; w++) {
      g_next += w < wave ? s_misc[2 + w] : 0u;
      total += s_misc[2 + w];
    }
    m = s_misc[1];
#pragma unroll
    for (uint32_t r = 0; r < kCollapseRowsPerThread; r++)
      if ((reps >> r) & 1u) s_tab[slot[r]] = g_next++;  // the slot now holds the group's number
    __syncthreads();

    // ---- 4. (group, row) keys, sorted: runs of groups in row order ----
#pragma unroll
    for (uint32_t r = 0; r < kCollapseRowsPerThread; r++)
      if (slot[r] != NONE) slot[r] = (s_tab[slot[r]] << RB) | (tid * per + r);
    __syncthreads();  // (the table is read: its first half becomes the key array)
#pragma unroll
    for (uint32_t r = 0; r < kCollapseRowsPerThread; r++) {
      const uint32_t i = tid * per + r;
      if (r < per && i < pn) s_key[i] = slot[r];
    }
    __syncthreads();
    for (uint32_t kk = 2; kk <= pn; kk <<= 1) {
      for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
        for (uint32_t t = tid; t < pn / 2u; t += NT) {
          const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;
          const uint32_t a = s_key[i], b = s_key[l];
          if ((a > b) == ((i & kk) == 0u)) {
            s_key[i] = b;
            s_key[l] = a;
          }
        }
        __syncthreads();
      }
    }
    for (uint32_t j = tid; j < m; j += NT) {
      const uint32_t g = s_key[j] >> RB;
      if (j == 0 || (s_key[j - 1u] >> RB) != g) s_start[g] = j;
    }
    __syncthreads();
  }

  // ---- the groups (zeros past n_groups; a failed query has none) ----
  const uint32_t ng = total < G ? total : G;
  auto run_of = [&](const uint32_t g, uint32_t &st, uint32_t &en) {
    st = s_start[g];
    en = g + 1u < total ? s_start[g + 1u] : m;
  };
  auto kept = [&](const uint32_t size) {  // inner hits of a group of `size` rows
    const uint32_t members = size - 1u;
    const uint32_t left = members > from ? members - from : 0u;
    return left < S ? left : S;
  };
  if (tid == 0) {
    side(kClNGroups)[q] = ng;
    side(kClTotal)[q] = total;
    side(kClStatus)[q] = failed ? 1u : 0u;
  }
  for (uint32_t g = tid; g < G; g += NT) {
    uint32_t row = 0, ord = 0, size = 0, doc = 0, seg = 0, cnt = 0;
    float score = 0.0f;
    if (g < ng) {
      uint32_t st, en;
      run_of(g, st, en);
      row = s_key[st] & RMASK;
      ord = s_ord[row];
      size = en - st;
      doc = odoc[row];
      seg = oseg[row];
      score = oscore[row];
      cnt = kept(size);
    }
    const size_t o = (size_t)q * G + g;
    side(kClRow)[o] = row;
    side(kClOrd)[o] = ord;
    side(kClSize)[o] = size;
    side(kClDoc)[o] = doc;
    side(kClSeg)[o] = seg;
    side(kClScore)[o] = __float_as_uint(score);
    side(kClInnerCount)[o] = cnt;
  }
  if (S == 0) return;

  // ---- 5. inner hits ----
  auto write_inner = [&](const uint32_t g, const uint32_t j, const bool have, const uint32_t row) {
    const size_t o = ((size_t)q * G + g) * S + j;
    side(kClInnerRow)[o] = have ? row : 0u;
    side(kClInnerDoc)[o] = have ? odoc[row] : 0u;
    side(kClInnerSeg)[o] = have ? oseg[row] : 0u;
    side(kClInnerScore)[o] = have ? __float_as_uint(oscore[row]) : 0u;
  };
  if (p.n_parts == 0) {  // in row order: a slice of the run
    for (uint32_t x = tid; x < G * S; x += NT) {
      const uint32_t g = x / S, j = x - g * S;
      bool have = false;
      uint32_t row = 0;
      if (g < ng) {
        uint32_t st, en;
        run_of(g, st, en);
        have = j < kept(en - st);
        if (have) row = s_key[st + 1u + from + j] & RMASK;
      }
      write_inner(g, j, have, row);
    }
    return;
  }
  // under the inner sort: a wave per group, lane l holds the l-th best member seen so far (all-ones: none; no
  // row's key is all-ones, its doc word is a doc id)
  constexpr uint32_t NW = kSortWords;
  const uint32_t L = from + S;  // <= 64
  for (uint32_t g = wave; g < G; g += NT / 64u) {
    uint32_t K[NW], krow = 0;
#pragma unroll
    for (uint32_t w = 0; w < NW; w++) K[w] = 0xFFFFFFFFu;
    uint32_t st = 0, en = 0;
    if (g < ng) run_of(g, st, en);
    for (uint32_t base = st + 1u; base < en; base += 64u) {
      const uint32_t pos = base + lane;
      const bool has = pos < en;
      const uint32_t row = has ? (s_key[pos] & RMASK) : 0u;
      uint32_t C[NW], W[NW];
#pragma unroll
      for (uint32_t w = 0; w < NW; w++) C[w] = 0xFFFFFFFFu;
      if (has) sorted_key(p, ordered_score(oscore[row]), oseg[row], odoc[row], C);
#pragma unroll
      for (uint32_t w = 0; w < NW; w++) W[w] = (uint32_t)__shfl((int)K[w], (int)(L - 1u), 64);
      // (the list's last as it is now: it only gets better, so a member that does not beat it never enters)
      uint64_t todo = __ballot(has && collapse_less(C, W));
      while (todo) {
        const uint32_t c = (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        uint32_t B[NW];
#pragma unroll
        for (uint32_t w = 0; w < NW; w++) B[w] = (uint32_t)__shfl((int)C[w], (int)c, 64);
        const uint32_t brow = (uint32_t)__shfl((int)row, (int)c, 64);
        const uint64_t after = __ballot(collapse_less(B, K));  // the lanes whose member comes after this one
        if (after == 0ull) continue;
        const uint32_t ins = (uint32_t)__builtin_ctzll(after);
#pragma unroll
        for (uint32_t w = 0; w < NW; w++) {
          const uint32_t up = (uint32_t)__shfl_up((int)K[w], 1, 64);
          K[w] = lane > ins ? up : (lane == ins ? B[w] : K[w]);
        }
        const uint32_t uprow = (uint32_t)__shfl_up((int)krow, 1, 64);
        krow = lane > ins ? uprow : (lane == ins ? brow : krow);
      }
    }
    const uint32_t cnt = g < ng ? kept(en - st) : 0u;
    if (lane >= from && lane < L) write_inner(g, lane - from, lane - from < cnt, krow);
  }
}

}  // namespace slg
