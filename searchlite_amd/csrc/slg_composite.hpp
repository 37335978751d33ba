// slg_composite.hpp — the composite aggregation (slg_batch_prepare_composite; CompositeCollector and
// finalize_composite, query/aggs/mod.rs:1689-1842, :3264-3368).  The bucket space is the cross product of the
// sources' key spaces, far beyond a dense table, but a request returns only the `size` smallest tuples at or above
// a lower bound.  A tuple is packed into one u64 (source 0 in the most significant bits, a slot number per source)
// whose integer order is the reference's tuple order.  Two kernels, one workgroup of 256 threads per query, behind
// agg_kernel, over the candidate region the batch's scoring kernel left, walked as agg_walk walks it:
//
// composite_select_kernel: the size + 1 smallest DISTINCT keys >= q_lower[q].  Each wave keeps in LDS a private
//   open-addressed set of u64 keys (CpSet, slg_cpset.hpp, shared with term_bucket_select_kernel; kCpMinCap <= cap, a power of two >= 2 * (size + 1)) and a threshold T, at
//   first ~0.  A key >= T is dropped with one compare; any other key is inserted if absent (an LDS compare-and-swap:
//   the set is the wave's own, so the lanes of one step that hold the same key settle it among themselves).  When
//   the set passes its fill limit (3/4 of cap) the wave alone compacts it: a bitonic sort of the table in LDS, the
//   size + 1 smallest kept in registers, T = the largest kept key + 1, the table cleared and the kept keys inserted
//   again.  After ONE __syncthreads the other waves leave their sorted lists where they are and wave 0 offers
//   their keys to its own set, as it offered the docs' (duplicates across waves meet in the set), sorts once more
//   and writes the answer.  No barrier inside the walk, nothing visible across workgroups.
//   Exactness: T only falls (every kept key is below the T it was inserted under).  A key dropped at some T is
//   >= T > size + 1 distinct keys the wave has seen, and every key it has seen is a key of the query; so a dropped
//   key is not among the size + 1 smallest distinct keys of the query.  A key that IS among them is never dropped,
//   by any wave, and survives every compaction (fewer than size + 1 keys are below it), so wave 0's final set holds
//   the size + 1 smallest (or all, when there are fewer).  The answer is a set: independent of the order of arrival,
//   the same on every run.
// composite_collect_kernel: the query's n_buckets sorted keys in LDS (<= 8 KB); the candidates are walked again and
//   every tuple of every doc is binary-searched; a hit in row r adds one to count cell r and runs every child
//   through agg_collect with cell = child.off + r * child.rows, what a child of any bucket root gets.  Tables in LDS
//   up to kAggLdsBytes, else the query's slice of the batch's composite tables, zeroed on the batch's stream.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_aggs.hpp"
#include "slg_cpset.hpp"
#include "slg_wave.hpp"

namespace slg {

constexpr uint32_t kCpMaxSources = 4;    // SLG_MAX_COMPOSITE_SOURCES
enum : uint32_t { kCpTerms = 0, kCpHistogram = 1 };

struct CompositeSourceDev {
  uint32_t kind, shift;
  uint32_t n_ords, pad;
  const uint32_t *ord_rank;  // terms: the slot of every ordinal, or null (the ordinal is the slot)
  double interval;
  long long first_id;        // histogram: the id of slot 0
  long long zero_slot;       // histogram: the slot of -0.0 (+0.0 follows, positive ids are shifted by one), or -1
  unsigned long long slots;
};

struct CompositeParams {
  AggParams a;  // the candidates; nodes / cols: the children (n_nodes of them); counts / stats / count_cells /
                // stats_cells: the composite's own tables (row 0 .. size of counts: the composite's count cells)
  const CompositeSourceDev *src;  // [n_sources]
  const ColumnDev *src_cols;      // [n_sources * n_segs]
  uint32_t n_sources, size, cap;
  const unsigned long long *q_lower;  // [nq] inclusive lower bounds
  unsigned long long *keys;           // [nq * size]
  uint32_t *n_buckets, *has_more;     // [nq]
  uint32_t *err;                      // the word behind has_more: ...
  const uint32_t *flag;               // ... the index's error word as the batch's last kernel left it
};

// The slot of value idx of a source's column; false: the value has none (an ordinal beyond the dictionary, an id
// outside the layout's range: registration and the recorded minimum and maximum rule both out)
__device__ __forceinline__ bool cp_slot(const CompositeSourceDev &s, const ColumnDev &col, const uint32_t idx,
                                        unsigned long long &slot) {
  if (s.kind == kCpTerms) {
    const uint32_t o = col.ords()[idx];
    if (o >= s.n_ords) return false;
    slot = s.ord_rank ? s.ord_rank[o] : o;
    return slot < s.slots;
  }
  // floor(v / interval): IEEE f64 division and floor (no fast-math); the key is that times interval, so its bits are
  // -0.0 exactly when the floor is -0.0
  const double f = floor(col.f64()[idx] / s.interval);
  long long sl;
  if (f == 0.0) {
    if (s.zero_slot < 0) return false;
    sl = s.zero_slot + (__double_as_longlong(f) < 0 ? 0 : 1);
  } else {
    if (!(f > -2147483648.0 && f < 2147483648.0)) return false;
    const long long id = (long long)f;
    sl = id - s.first_id + ((id > 0 && s.zero_slot >= 0) ? 1 : 0);
  }
  if (sl < 0 || (unsigned long long)sl >= s.slots) return false;
  slot = (unsigned long long)sl;
  return true;
}

// The first value at or behind `from` of the doc's values [a, e) that has a slot no earlier value of the doc has
// (distinct slots per source give distinct tuples: the reference's dedup of the combinations); e: none
__device__ __forceinline__ uint32_t cp_next(const CompositeSourceDev &s, const ColumnDev &col, const uint32_t a,
                                            const uint32_t from, const uint32_t e, unsigned long long &slot) {
  for (uint32_t i = from; i < e; i++) {
    unsigned long long x;
    if (!cp_slot(s, col, i, x)) continue;
    bool dup = false;
    for (uint32_t j = a; j < i; j++) {
      unsigned long long y;
      dup = dup || (cp_slot(s, col, j, y) && y == x);
    }
    if (dup) continue;
    slot = x;
    return i;
  }
  return e;
}

// The tuples of one doc, one at a time: an odometer over the sources' distinct slots, the last source fastest.
// (every loop over the sources is unrolled with constant indices: the state stays in registers)
struct CpTuples {
  uint32_t a[kCpMaxSources], e[kCpMaxSources], i[kCpMaxSources], first[kCpMaxSources];
  unsigned long long part[kCpMaxSources], first_part[kCpMaxSources];
  bool live;
  // a doc without a value in any one source has no tuple
  __device__ __forceinline__ void start(const CompositeParams &p, const bool ok, const uint32_t seg, const uint32_t doc) {
    live = ok;
#pragma unroll
    for (uint32_t s = 0; s < kCpMaxSources; s++) {
      a[s] = e[s] = i[s] = first[s] = 0u;
      part[s] = first_part[s] = 0ull;
      if (s < p.n_sources && live) {
        const CompositeSourceDev &src = p.src[s];
        const ColumnDev col = p.src_cols[(size_t)s * p.a.n_segs + seg];
        column_range(col, doc, a[s], e[s]);
        unsigned long long slot = 0;
        i[s] = first[s] = cp_next(src, col, a[s], a[s], e[s], slot);
        part[s] = first_part[s] = slot << src.shift;
        live = i[s] < e[s];
      }
    }
  }
  __device__ __forceinline__ unsigned long long key() const {
    unsigned long long k = 0;
#pragma unroll
    for (uint32_t s = 0; s < kCpMaxSources; s++) k |= part[s];
    return k;
  }
  __device__ __forceinline__ void advance(const CompositeParams &p, const uint32_t seg) {
    bool carry = true;
#pragma unroll
    for (uint32_t r = 0; r < kCpMaxSources; r++) {
      const uint32_t s = kCpMaxSources - 1u - r;
      if (s < p.n_sources && carry) {
        const CompositeSourceDev &src = p.src[s];
        const ColumnDev col = p.src_cols[(size_t)s * p.a.n_segs + seg];
        unsigned long long slot = 0;
        const uint32_t nx = cp_next(src, col, a[s], i[s] + 1u, e[s], slot);
        if (nx < e[s]) {
          i[s] = nx;
          part[s] = slot << src.shift;
          carry = false;
        } else {
          i[s] = first[s];
          part[s] = first_part[s];
        }
      }
    }
    if (carry) live = false;
  }
};

static __global__ void __launch_bounds__(kCpThreads) composite_select_kernel(CompositeParams p) {
  extern __shared__ unsigned long long cp_lds[];  // the four waves' sets
  __shared__ uint32_t sh_n[kCpWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t q = blockIdx.x;
  if (q >= p.a.nq) return;
  const QueryRef qr = p.a.queries[q];
  const uint32_t flt = p.a.q_filter ? p.a.q_filter[q] : 0u;
  const unsigned long long lower = p.q_lower[q];
  if (q == 0 && tid == 0) *p.err = *p.flag;
  CpSet set{cp_lds + (size_t)wave * p.cap, p.cap, p.size, 0u, kCpEmpty};
  set.clear(lane);

  agg_walk<true>(p.a, qr, flt, wave, lane, [&](const bool ok, const uint32_t seg, const uint32_t doc) {
    CpTuples t;
    t.start(p, ok, seg, doc);
    while (__ballot(t.live)) {  // a step: at most one key per lane
      const unsigned long long key = t.key();
      set.offer(t.live && key >= lower, key, lane);
      if (t.live) t.advance(p, seg);
    }
  });
  if (wave != 0u) {
    set.sort(lane);
    if (lane == 0) sh_n[wave] = set.count < p.size + 1u ? set.count : p.size + 1u;
  }
  __syncthreads();
  if (wave != 0u) return;
  for (uint32_t w = 1; w < kCpWaves; w++) {
    const unsigned long long *L = cp_lds + (size_t)w * p.cap;
    const uint32_t n = sh_n[w];
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
      const bool has = i0 + lane < n;
      set.offer(has, has ? L[i0 + lane] : kCpEmpty, lane);
    }
  }
  set.sort(lane);
  const uint32_t nb = set.count < p.size ? set.count : p.size;
  unsigned long long *out = p.keys + (size_t)q * p.size;
  for (uint32_t i = lane; i < p.size; i += 64) out[i] = i < nb ? set.H[i] : 0ull;
  if (lane == 0) {
    p.n_buckets[q] = nb;
    p.has_more[q] = set.count > p.size ? 1u : 0u;
  }
}

template <bool LDS, bool EXT>
static __global__ void __launch_bounds__(kCpThreads) composite_collect_kernel(CompositeParams p) {
  extern __shared__ unsigned long long cc_lds[];  // the selected keys [size], then (LDS) the stats cells, the count cells
  __shared__ uint32_t sh_matched;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t q = blockIdx.x;
  if (q >= p.a.nq) return;
  const QueryRef qr = p.a.queries[q];
  const uint32_t flt = p.a.q_filter ? p.a.q_filter[q] : 0u;
  const uint32_t nb = p.n_buckets[q];
  unsigned long long *const sk = cc_lds;
  unsigned long long *const tab = cc_lds + p.size;
  AggStatDev *st = LDS ? reinterpret_cast<AggStatDev *>(tab) : p.a.stats + (size_t)q * p.a.stats_cells;
  uint32_t *cnt = LDS ? reinterpret_cast<uint32_t *>(tab + 4 * (size_t)p.a.stats_cells)
                      : p.a.counts + (size_t)q * p.a.count_cells;
  if (tid == 0) sh_matched = 0;
  for (uint32_t i = tid; i < nb; i += kCpThreads) sk[i] = p.keys[(size_t)q * p.size + i];
  if (LDS) {
    const uint32_t words = 8 * p.a.stats_cells + p.a.count_cells;  // every cell starts as zero words
    uint32_t *w = reinterpret_cast<uint32_t *>(tab);
    for (uint32_t i = tid; i < words; i += kCpThreads) w[i] = 0u;
  }
  __syncthreads();

  uint32_t nv = 0;
  agg_walk<false>(p.a, qr, flt, wave, lane, [&](bool, const uint32_t seg, const uint32_t doc) {
    nv++;
    if (nb == 0u) return;
    CpTuples t;
    for (t.start(p, true, seg, doc); t.live; t.advance(p, seg)) {
      const unsigned long long key = t.key();
      uint32_t lo = 0, hi = nb;  // the first row whose key is >= key
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sk[mid] < key) lo = mid + 1u;
        else hi = mid;
      }
      if (lo == nb || sk[lo] != key) continue;
      atomicAdd(&cnt[lo], 1u);
      for (uint32_t c = 0; c < p.a.n_nodes; c++) {
        const AggNodeDev &ch = p.a.nodes[c];
        agg_collect<EXT>(p.a, ch, seg, doc, ch.off + lo * ch.rows, cnt, st, [](uint32_t) {});
      }
    }
  });
  nv = wave_sum(nv);
  if (lane == 0 && nv) atomicAdd(&sh_matched, nv);
  __syncthreads();
  if (tid == 0 && p.a.out_matched) p.a.out_matched[q] = sh_matched;
  if (LDS) {
    uint32_t *oc = p.a.counts + (size_t)q * p.a.count_cells;
    for (uint32_t i = tid; i < p.a.count_cells; i += kCpThreads) oc[i] = cnt[i];
    unsigned long long *os = reinterpret_cast<unsigned long long *>(p.a.stats + (size_t)q * p.a.stats_cells);
    for (uint32_t i = tid; i < 4 * p.a.stats_cells; i += kCpThreads) os[i] = tab[i];
  }
}

}  // namespace slg
