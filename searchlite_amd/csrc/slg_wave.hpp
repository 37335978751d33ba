// slg_wave.hpp — device-side building blocks shared by every kernel of the library: small wave
// helpers (readlanes, scans, fences, one LDS atomic per wave: hist_add_by_bin, wave_compact_slot), the
// register top-k WaveTopK (insert, the stream-and-insert loop `offer`, the result row `store_row`), the
// buffered top-k BufTopK, the readers of a registered column (column_range, sorted_key), and the three scalar
// rules of a vector score (missing_vector_score, similarity_from_sum, blend) that the rerank and the
// vector-search kernels restate from the reference.
// Device code and two launch helpers (launch_with_lds, with_kregs), no kernels: the scoring units
// (slg_score_inst.hip) include it without compiling a copy of the host-launched kernels of slg_kernels.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "slg_desc.hpp"

namespace slg {

typedef float f32x4_t __attribute__((ext_vector_type(4)));  // 16-byte lane loads, MFMA accumulators

// ---- small helpers --------------------------------------------------------------------
__device__ __forceinline__ int32_t total_key(float x) {
  // f32::total_cmp key: sign-magnitude bits -> two's complement order
  int32_t b = __float_as_int(x);
  return b ^ (int32_t)(((uint32_t)(b >> 31)) >> 1);
}
__device__ __forceinline__ float key_to_float(int32_t k) {
  return __int_as_float(k ^ (int32_t)(((uint32_t)(k >> 31)) >> 1));
}
__device__ __forceinline__ uint32_t rfl(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ uint32_t rl(uint32_t v, uint32_t lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  return ((uint64_t)rfl((uint32_t)(v >> 32)) << 32) | rfl((uint32_t)v);
}
// *src read through the constant address space (scalar loads when the address is wave-uniform): for
// data written before the kernel starts and never during it
template <typename T>
__device__ __forceinline__ T load_const(const T *src) {
  static_assert(sizeof(T) % 4 == 0, "whole words");
  typedef const __attribute__((address_space(4))) uint32_t *c_u32_t;
  const c_u32_t w = (c_u32_t)(uintptr_t)src;
  T out;
  uint32_t *dst = reinterpret_cast<uint32_t *>(&out);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 4; i++) dst[i] = w[i];
  return out;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    uint32_t u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t lane) {
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t u = __shfl_up(x, o, 64);
    if (lane >= (uint32_t)o) x += u;
  }
  return x - v;
}
// lane l receives lane l-1's value (lane 0 keeps its own): one DPP move, no LDS traffic
__device__ __forceinline__ int32_t wave_shr1(int32_t v) {
  return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
// wave-wide f32 sum with DPP row shifts / broadcasts (no LDS round trips); result in lane 63
__device__ __forceinline__ float wave_sum_f(float v) {
  int x = __float_as_int(v);
#define SLG_DPP_ADD(ctrl, rmask)                                                                \
  x = __float_as_int(__int_as_float(x) +                                                        \
                     __int_as_float(__builtin_amdgcn_update_dpp(0, x, ctrl, rmask, 0xf, true)))
  SLG_DPP_ADD(0x111, 0xf);  // row_shr:1
  SLG_DPP_ADD(0x112, 0xf);  // row_shr:2
  SLG_DPP_ADD(0x114, 0xf);  // row_shr:4
  SLG_DPP_ADD(0x118, 0xf);  // row_shr:8
  SLG_DPP_ADD(0x142, 0xa);  // row_bcast:15
  SLG_DPP_ADD(0x143, 0xc);  // row_bcast:31
#undef SLG_DPP_ADD
  return __int_as_float(__builtin_amdgcn_readlane(x, 63));
}

// compiler-only ordering point for wave-synchronous LDS traffic (hardware keeps a wave's
// DS instructions in order; this stops the compiler from moving them across phases)
__device__ __forceinline__ void wave_fence() { __atomic_signal_fence(__ATOMIC_SEQ_CST); }

// hist[bin] += 1 for every lane that is here, one LDS atomic per DISTINCT bin of the wave: LDS atomics
// on one address are served one at a time, and the lanes of a wave mostly hold the same one or two bins
__device__ __forceinline__ void hist_add_by_bin(uint32_t *hist, const uint32_t bin, const uint32_t lane) {
  uint64_t todo = __ballot(true);  // the lanes that are here
  while (todo) {
    const uint32_t l = (uint32_t)__builtin_ctzll(todo);
    const uint32_t b = rl(bin, l);
    const uint64_t same = __ballot(bin == b) & todo;
    if (lane == l) atomicAdd(&hist[b], (uint32_t)__popcll(same));
    todo &= ~same;
  }
}
// compaction slot of every lane with `win` set: one atomicAdd on *counter per wave (by its first winning
// lane), then the lane's rank among the winners.  Lanes without `win` get a value they must not use.
__device__ __forceinline__ uint32_t wave_compact_slot(uint32_t *counter, const bool win, const uint32_t lane) {
  const uint64_t wm = __ballot(win);
  uint32_t wbase = 0;
  if (wm != 0ull) {
    const uint32_t l0 = (uint32_t)__builtin_ctzll(wm);
    if (lane == l0) wbase = atomicAdd(counter, (uint32_t)__popcll(wm));
    wbase = rl(wbase, l0);
  }
  return wbase + (uint32_t)__popcll(wm & ((1ull << lane) - 1ull));
}

// (score key, seg, doc) ordering: larger tk first, then smaller seg, then smaller doc
// (query/wand.rs:30-37, query/sort.rs:80-93)
template <bool HAS_SEG>
__device__ __forceinline__ bool better(int32_t tka, uint32_t sega, uint32_t doca, int32_t tkb,
                                       uint32_t segb, uint32_t docb) {
  if (tka != tkb) return tka > tkb;
  if (HAS_SEG && sega != segb) return sega < segb;
  return doca < docb;
}

// ---- wave-wide sorted top-k held in registers -------------------------------------------
// Position p = lane*KREGS + r (best first).  Capacity 64*KREGS >= k.  All methods are
// wave-uniform in control flow; candidates are passed as uniform (SGPR) values.
template <int KREGS, bool HAS_SEG>
struct WaveTopK {
  int32_t tk[KREGS];
  uint32_t doc[KREGS];
  uint32_t seg[HAS_SEG ? KREGS : 1];
  int32_t th_tk;  // threshold = entry at position k-1 (uniform), never below the floor
  uint32_t th_seg, th_doc;
  uint32_t count;  // real entries held, capped at k (uniform)
  int32_t floor_tk;  // exact lower bound of the final k-th score known up front (or sentinel)

  __device__ __forceinline__ void init() {
#pragma unroll
    for (int r = 0; r < KREGS; r++) {
      tk[r] = kSentinelTk;
      doc[r] = 0xFFFFFFFFu;
      if (HAS_SEG) seg[r] = 0xFFFFFFFFu;
    }
    if (!HAS_SEG) seg[0] = 0;
    th_tk = kSentinelTk;
    th_seg = 0xFFFFFFFFu;
    th_doc = 0xFFFFFFFFu;
    count = 0;
    floor_tk = kSentinelTk;
  }
  // At least k docs are known to score >= f: nothing below f can reach the final top-k.
  // Candidates equal to f still pass (ties are broken by doc id later).
  __device__ __forceinline__ void set_floor(float f) {
    floor_tk = total_key(f);
    th_tk = floor_tk;
    th_seg = 0xFFFFFFFFu;
    th_doc = 0xFFFFFFFFu;
  }
  __device__ __forceinline__ bool passes(int32_t ctk, uint32_t cseg, uint32_t cdoc) const {
    return better<HAS_SEG>(ctk, cseg, cdoc, th_tk, th_seg, th_doc);
  }
  // insert a uniform candidate known to pass the threshold
  __device__ __forceinline__ void insert(int32_t ctk, uint32_t cseg, uint32_t cdoc, uint32_t k,
                                         uint32_t lane) {
    uint32_t cnt = 0;
#pragma unroll
    for (int r = 0; r < KREGS; r++)
      cnt += better<HAS_SEG>(tk[r], HAS_SEG ? seg[r] : 0u, doc[r], ctk, cseg, cdoc) ? 1u : 0u;
    uint64_t full = __ballot(cnt == (uint32_t)KREGS);
    uint32_t pos_lane = (uint32_t)__popcll(full);  // fully-better lanes form a prefix
    uint32_t pos_r = pos_lane < 64 ? rl(cnt, pos_lane) : 0u;
    // value arriving from the previous lane's last register
    int32_t up_tk = wave_shr1(tk[KREGS - 1]);
    uint32_t up_doc = (uint32_t)wave_shr1((int32_t)doc[KREGS - 1]);
    uint32_t up_seg = HAS_SEG ? (uint32_t)wave_shr1((int32_t)seg[KREGS - 1]) : 0u;
#pragma unroll
    for (int r = KREGS - 1; r >= 0; r--) {
      bool shift = lane > pos_lane || (lane == pos_lane && (uint32_t)r > pos_r);
      bool here = lane == pos_lane && (uint32_t)r == pos_r;
      int32_t s_tk = r == 0 ? up_tk : tk[r > 0 ? r - 1 : 0];
      uint32_t s_doc = r == 0 ? up_doc : doc[r > 0 ? r - 1 : 0];
      uint32_t s_seg = HAS_SEG ? (r == 0 ? up_seg : seg[r > 0 ? r - 1 : 0]) : 0u;
      tk[r] = here ? ctk : (shift ? s_tk : tk[r]);
      doc[r] = here ? cdoc : (shift ? s_doc : doc[r]);
      if (HAS_SEG) seg[r] = here ? cseg : (shift ? s_seg : seg[r]);
    }
    if (count < k) count++;
    // refresh threshold = entry at position k-1
    uint32_t tl = (k - 1) / KREGS, tr = (k - 1) % KREGS;
    int32_t v_tk = tk[0];
    uint32_t v_doc = doc[0], v_seg = HAS_SEG ? seg[0] : 0u;
#pragma unroll
    for (int r = 1; r < KREGS; r++) {
      bool sel = tr == (uint32_t)r;
      v_tk = sel ? tk[r] : v_tk;
      v_doc = sel ? doc[r] : v_doc;
      if (HAS_SEG) v_seg = sel ? seg[r] : v_seg;
    }
    th_tk = (int32_t)rl((uint32_t)v_tk, tl);
    th_doc = rl(v_doc, tl);
    th_seg = HAS_SEG ? rl(v_seg, tl) : 0u;
    if (th_tk < floor_tk) {  // fewer than k entries so far: the up-front bound still rules
      th_tk = floor_tk;
      th_doc = 0xFFFFFFFFu;
      th_seg = 0xFFFFFFFFu;
    }
  }
  // one candidate per lane (`valid`: the lane holds one): the passing lanes are taken lowest first, each
  // inserted through readlanes, and the rest re-balloted against the threshold the insert raised
  __device__ __forceinline__ void offer(bool valid, int32_t ctk, uint32_t cseg, uint32_t cdoc, uint32_t k,
                                        uint32_t lane) {
    uint64_t m = __ballot(valid && passes(ctk, cseg, cdoc));
    while (m) {
      const uint32_t l = (uint32_t)__builtin_ctzll(m);
      insert((int32_t)rl((uint32_t)ctk, l), rl(cseg, l), rl(cdoc, l), k, lane);
      m &= m - 1;
      m &= __ballot(passes(ctk, cseg, cdoc));
    }
  }
  // the result row of query q: k entries best first, zeros behind the real ones, and their count
  __device__ __forceinline__ void store_row(uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                                            uint32_t *out_count, uint32_t q, uint32_t k, uint32_t lane) const {
#pragma unroll
    for (int r = 0; r < KREGS; r++) {
      const uint32_t pos = lane * KREGS + r;
      if (pos < k) {
        const bool real = pos < count;
        out_doc[(size_t)q * k + pos] = real ? doc[r] : 0u;
        out_seg[(size_t)q * k + pos] = real ? seg[r] : 0u;
        out_score[(size_t)q * k + pos] = real ? key_to_float(tk[r]) : 0.0f;
      }
    }
    if (lane == 0) out_count[q] = count;
  }
};

// ---- buffered wave top-k (one segment) ------------------------------------------------------
// push_top_k (query/wand.rs:905-916) without a per-candidate sorted insert: a candidate that
// beats the current threshold is appended to a per-wave LDS buffer (one ds_write for all passing
// lanes of a slot); only when the buffer is full, and once at the end, are the entries ranked
// (every lane counts the entries better than its own) and the k best kept.  The threshold is
// the k-th best after a ranking, the up-front floor before, so it is always a valid lower bound
// of the final k-th score: the surviving set is exactly the top-k under (score desc, doc asc).
//
// Entries are single 64-bit keys: (order-preserving score bits << 32) | ~doc, so "better" is
// one unsigned 64-bit compare.
__device__ __forceinline__ uint32_t ordered_score(float x) {
  const int32_t b = __float_as_int(x);  // == total_key(x) ^ 0x80000000
  return (uint32_t)b ^ ((uint32_t)(b >> 31) | 0x80000000u);
}
__device__ __forceinline__ uint64_t cand_key(float score, uint32_t doc) {
  return ((uint64_t)ordered_score(score) << 32) | (uint32_t)~doc;
}

// ---- registered columns (slg_desc.hpp: ColumnDev, SortColDev) -------------------------------------
// the values of `doc` in a column are vals[a .. e)
__device__ __forceinline__ void column_range(const ColumnDev &c, const uint32_t doc, uint32_t &a, uint32_t &e) {
  a = c.offs ? c.offs[doc] : doc;
  e = c.offs ? c.offs[doc + 1u] : doc + 1u;
}
// The sort key of (seg, doc) under the sort that p describes (its layout: slg_kernels.hpp, the field-sorted
// select): p.sort_cols[part * p.n_segs + seg], p.n_parts, and bit i of p.score_parts / p.desc_parts for part i.
// a: the doc's ordered score, what a `_score` part holds
template <typename P>
__device__ __forceinline__ void sorted_key(const P &p, const uint32_t a, const uint32_t seg, const uint32_t doc,
                                           uint32_t (&K)[kSortWords]) {
#pragma unroll
  for (uint32_t i = 0; i < kSortMaxParts; i++) {
    uint32_t w0 = 0, w1 = 0, w2 = 0;
    if (i < p.n_parts) {
      if ((p.score_parts >> i) & 1u) {
        w2 = ((p.desc_parts >> i) & 1u) ? ~a : a;
      } else {
        const SortColDev c = p.sort_cols[(size_t)i * p.n_segs + seg];
        const uint32_t pw = c.present[doc >> 5];
        const unsigned long long v = c.key[doc];  // (0 for a Missing doc)
        w0 = ((pw >> (doc & 31u)) & 1u) ^ 1u;
        w1 = (uint32_t)(v >> 32);
        w2 = (uint32_t)v;
      }
    }
    K[3 * i] = w0;
    K[3 * i + 1] = w1;
    K[3 * i + 2] = w2;
  }
  K[kSortWords - 2] = seg;
  K[kSortWords - 1] = doc;
}

// ---- the scalar rules of a vector score (rerank and vector-only search) -------------------------
// api/reader.rs:217-223: what a doc without a vector scores, by the field's metric (0 cosine, else L2)
__device__ __forceinline__ float missing_vector_score(const int32_t metric) {
  return metric == 0 ? -1.0f : -3.40282347e+38f;
}
// metric_similarity (vectors/mod.rs:107-120) from the finished sum: cosine = the dot, NaN -> 0 (:112-116);
// L2 = -sqrt of the sum of squared differences (:118)
__device__ __forceinline__ float similarity_from_sum(const int32_t metric, const float sum) {
  return metric == 0 ? ((sum != sum) ? 0.0f : sum) : -sqrtf(sum);
}
// blend_scores of one clause (api/reader.rs:240-246, vectors/mod.rs:122-129)
__device__ __forceinline__ float blend(const float alpha, const float bm, const float vs) {
  if (alpha >= 1.0f) return bm;
  if (alpha <= 0.0f) return vs;
  return alpha * bm + (1.0f - alpha) * vs;  // vectors/mod.rs:128
}

template <int KREGS>
struct BufTopK {
  static constexpr uint32_t kEntries = 64u * (KREGS + 1);  // >= k + 64 for k <= 64 * KREGS: after a
                                                          // ranking a whole slot of candidates fits
  static constexpr int E = KREGS + 1;                      // entries per lane while ranking
  uint64_t *buf;   // LDS [kEntries]
  uint32_t count;  // uniform: entries held
  uint64_t th;     // uniform: a candidate passes iff key > th

  __device__ __forceinline__ void init(uint64_t *lds) {
    buf = lds;
    count = 0;
    th = 0;  // any real doc passes (~doc > 0)
  }
  // At least k docs score >= f.  Candidates equal to f still pass (doc-id tie break later).
  __device__ __forceinline__ void set_floor(float f) {
    th = ((uint64_t)ordered_score(f) << 32) - 1ull;
  }
  __device__ __forceinline__ bool passes(uint64_t key) const { return key > th; }

  // drop deleted docs (accept(), query/wand.rs:905), rank the rest, keep the k best sorted at
  // buf[0..count), refresh the threshold.  Deleted docs are filtered here, before anything is
  // ranked, so they never influence the threshold.
  __device__ __forceinline__ void compact(uint32_t k, uint32_t lane, const uint32_t *deleted) {
    uint64_t e[E];
    uint32_t rank[E];
#pragma unroll
    for (int i = 0; i < E; i++) {
      const uint32_t idx = lane + 64u * i;
      e[i] = idx < count ? buf[idx] : 0ull;
      rank[i] = 0;
    }
    if (deleted) {
#pragma unroll
      for (int i = 0; i < E; i++) {
        const uint32_t doc = ~(uint32_t)e[i];
        if (e[i] != 0ull && ((deleted[doc >> 5] >> (doc & 31)) & 1u)) e[i] = 0ull;
      }
    }
    uint32_t nvalid = 0;
#pragma unroll
    for (int i = 0; i < E; i++) {
      if (64u * i < count) {  // uniform
        nvalid += (uint32_t)__popcll(__ballot(e[i] != 0ull));
        const uint32_t n_i = count - 64u * i < 64u ? count - 64u * i : 64u;
        for (uint32_t l = 0; l < n_i; l++) {
          const uint64_t c = ((uint64_t)rl((uint32_t)(e[i] >> 32), l) << 32) | rl((uint32_t)e[i], l);
#pragma unroll
          for (int j = 0; j < E; j++) rank[j] += c > e[j] ? 1u : 0u;
        }
      }
    }
    wave_fence();
#pragma unroll
    for (int i = 0; i < E; i++)
      if (e[i] != 0ull && rank[i] < k) buf[rank[i]] = e[i];
    wave_fence();
    count = nvalid < k ? nvalid : k;
    if (nvalid >= k) {
      const uint64_t kth = buf[k - 1];
      const uint64_t u = ((uint64_t)rfl((uint32_t)(kth >> 32)) << 32) | rfl((uint32_t)kth);
      th = u > th ? u : th;
    }
  }

  // split-key forms (the hot path keeps 32-bit halves: hi = ordered score, lo = ~doc)
  __device__ __forceinline__ bool passes(uint32_t hi, uint32_t lo) const {
    const uint32_t th_hi = (uint32_t)(th >> 32), th_lo = (uint32_t)th;
    return hi > th_hi || (hi == th_hi && lo > th_lo);
  }
  // append the candidates of the lanes with `pass` set (pass implies key > th); the caller
  // has checked that they fit (count + popcount <= kEntries)
  __device__ __forceinline__ void append(bool pass, uint32_t hi, uint32_t lo, uint32_t lane) {
    const uint64_t m = __ballot(pass);
    if (m == 0ull) return;
    const uint32_t dest =
        count + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    uint32_t *b32 = reinterpret_cast<uint32_t *>(buf);
    if (pass) {
      b32[2 * dest] = lo;
      b32[2 * dest + 1] = hi;
    }
    count += (uint32_t)__popcll(m);
  }
  // same, ranking first when the buffer would overflow (<= 64 candidates always fit after it)
  __device__ __forceinline__ void append_checked(bool pass, uint32_t hi, uint32_t lo, uint32_t k,
                                                 uint32_t lane, const uint32_t *deleted) {
    if (count + (uint32_t)__popcll(__ballot(pass)) > kEntries) {
      compact(k, lane, deleted);
      pass = pass && passes(hi, lo);
    }
    append(pass, hi, lo, lane);
  }

  // final candidates of this wave: k entries (int32 total_key, doc), sentinel padded (best
  // first when they were ranked; the merge does not rely on the order)
  __device__ __forceinline__ void write_out(int32_t *otk, uint32_t *odoc, uint32_t k, uint32_t lane,
                                            const uint32_t *deleted) {
    if (count > k || (deleted && count)) compact(k, lane, deleted);
    wave_fence();
#pragma unroll
    for (int r = 0; r < KREGS; r++) {
      const uint32_t pos = lane + 64u * r;
      if (pos < k) {
        const uint64_t e = pos < count ? buf[pos] : 0ull;
        otk[pos] = pos < count ? (int32_t)((uint32_t)(e >> 32) ^ 0x80000000u) : kSentinelTk;
        odoc[pos] = ~(uint32_t)e;
      }
    }
  }
};

// ---- launch helpers of the one-workgroup-per-query kernels (rerank, rescore) ------------------------
template <typename K, typename P>
inline hipError_t launch_with_lds(K kernel, const P &params, uint32_t nq, size_t lds, hipStream_t st) {
  if (lds > 48 * 1024) {  // above the default dynamic-LDS limit: opt in (up to the CU's 160 KiB)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, dim3(nq), dim3(256), lds, st, params);
  return hipGetLastError();
}

// launch(std::integral_constant<int, KREGS>{}) for the top-k register width kregs names: a kernel launched
// through it is instantiated for KREGS 1, 2, 4, 8 and 16
template <typename F>
inline hipError_t with_kregs(int kregs, F &&launch) {
  switch (kregs) {
    case 1: return launch(std::integral_constant<int, 1>{});
    case 2: return launch(std::integral_constant<int, 2>{});
    case 4: return launch(std::integral_constant<int, 4>{});
    case 8: return launch(std::integral_constant<int, 8>{});
    default: return launch(std::integral_constant<int, 16>{});
  }
}

}  // namespace slg
