// slg_vsearch.hpp — exact vector-only search over every stored vector (the device form of
// search_vector_only, searchlite-core/src/api/reader.rs:2187-2330, with the per-segment HNSW search of
// collect_vector_maps, :2379-2469, replaced by an exact scan).
//
// Per clause, a scan scores tiles of 64 queries x 128 docs (the docs of all segments form one flat
// space, flat = doc_base[seg] + doc, so flat order is (segment asc, doc asc)).  Cosine runs on the f32
// matrix cores (v_mfma_f32_16x16x4_f32, an fmaf chain over the dimension); L2 is the direct
// sum (x - y)^2 on the VALU over the same LDS tiles (the |x|^2 + |y|^2 - 2 x.y form cancels for
// near-duplicates).  Candidates are 64-bit keys (ordered score << 32) | ~flat: one unsigned compare
// orders them by (score desc, segment asc, doc asc), f32::total_cmp as the reference's sort.
//
//   cand_size <= kVsSmallK: the scan keeps each query's running top-cand_size in an LDS buffer per
//     query (append what beats the threshold, rank when full) and writes one partial list per doc
//     chunk; vs_select_kernel merges the partials.  No score matrix goes to HBM.
//   larger cand_size: the scan writes the keys of a chunk of docs, vs_select_kernel folds the chunk
//     into each query's running top-cand_size (bitonic sort in LDS), chunk after chunk.
// vs_select_kernel's last step also leaves every clause list sorted by doc; vs_blend_kernel forms the
// union of the clause lists, applies compute_hybrid_score at bm25 = 0 (:225-254) and sorts the union.
// Hybrid text + vector search (slg_hybrid.hpp) gathers its keys from a batch's matched docs and shares the
// last two steps: vs_select_kernel folds them, vs_blend_kernel<true> adds the BM25 hits to the union.
//
// What the scans of the family share lives here: vs_tile_scores (the f32 tile body of vs_scan_kernel and of the
// cosine IVF scan), VsEpilogue / vs_tile_topk / vs_write_partials (the fused top-k epilogue of those two and of the bf16 first
// pass; the flat id of a tile row and the slot of a partial list are functors) and VsReject.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_wave.hpp"

namespace slg {

constexpr uint32_t kVsTileDocs = 128;  // docs of a scan tile
constexpr uint32_t kVsTileQ = 64;      // queries of a scan tile (16 per wave)
constexpr uint32_t kVsKc = 32;         // dimensions staged in LDS at a time (zero-padded)
constexpr uint32_t kVsRow = 36;        // LDS row of a tile (floats, padded against bank conflicts)
constexpr uint32_t kVsSmallK = 64;     // cand_size up to this: fused top-k epilogue
constexpr uint32_t kVsBufCap = 96;     // epilogue buffer entries per query (cand_size <= 64)
constexpr uint32_t kVsBufCapNarrow = 40;  // ... for cand_size <= 32: 49 KiB of LDS, three workgroups per CU
constexpr uint32_t kVsSortCap = 16384; // keys sorted in LDS by the select / blend kernels
constexpr uint32_t kVsSortThreads = 1024;

struct VsScanParams {
  const VecSegDev *vsegs;                // the clause field's per-segment stores
  const SegDev *segs;                    // per-segment tombstones
  const uint32_t *const *reject_table;   // [n_filters * n_segs] reject bitmaps (deleted | ~filter)
  const uint32_t *doc_base;              // [n_segs + 1] first flat doc of each segment
  uint32_t n_segs, n_filters, dim, nq;
  const float *qvecs;                    // query q's clause vector: qvecs + q * q_stride + q_off
  uint32_t q_stride, q_off, qvec4;       // qvec4: 16-byte query loads are aligned
  const float *boost;                    // [nq][n_clauses] or nullptr
  uint32_t n_clauses, clause;
  const int32_t *q_filter;               // [nq] < 0 none, or nullptr
  uint32_t tile_begin, tile_end, tiles_per_block;
  uint64_t *out;     // top-k: [(q * n_chunks + chunk) * kVsSmallK]; store: [q * out_stride + flat - tile_begin * 128]
  uint32_t out_stride, n_chunks, k;
  uint32_t cap;      // (top-k) epilogue buffer entries per query: kVsBufCap or kVsBufCapNarrow
};

__device__ __forceinline__ float vs_key_score(uint64_t key) {
  const uint32_t hi = (uint32_t)(key >> 32);
  return __int_as_float((int32_t)((hi & 0x80000000u) ? (hi ^ 0x80000000u) : ~hi));
}

__device__ __forceinline__ uint32_t vs_seg_of(const uint32_t *doc_base, uint32_t n_segs, uint32_t flat) {
  uint32_t lo = 0, hi = n_segs;  // last segment whose base is <= flat
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (doc_base[mid] <= flat)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// rank the entries of one query's buffer, keep the k best sorted at b[0..), return how many are kept
// (wave-wide; n <= 128 valid, distinct, non-zero keys)
__device__ __forceinline__ uint32_t vs_compact(uint64_t *b, uint32_t n, uint32_t k, uint32_t lane) {
  const uint64_t e0 = lane < n ? b[lane] : 0ull, e1 = lane + 64 < n ? b[lane + 64] : 0ull;
  uint32_t r0 = 0, r1 = 0;
  for (uint32_t l = 0; l < n; l++) {
    const uint64_t src = l < 64 ? e0 : e1;
    const uint32_t sl = l & 63u;
    const uint64_t c = ((uint64_t)rl((uint32_t)(src >> 32), sl) << 32) | rl((uint32_t)src, sl);
    r0 += c > e0 ? 1u : 0u;
    r1 += c > e1 ? 1u : 0u;
  }
  wave_fence();
  if (e0 != 0ull && r0 < k) b[r0] = e0;
  if (e1 != 0ull && r1 < k) b[r1] = e1;
  wave_fence();
  return n < k ? n : k;
}

// one float4 of a row at dimension kk (zeros past dim or for a missing row)
__device__ __forceinline__ f32x4_t vs_ld4(const float *row, uint32_t kk, uint32_t dim, bool vec4) {
  const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
  if (!row) return z;
  typedef const __attribute__((address_space(1))) float *gf_t;
  typedef const __attribute__((address_space(1))) f32x4_t *gv_t;
  if (vec4) return kk < dim ? *(gv_t)((gf_t)row + kk) : z;
  const gf_t r = (gf_t)row;
  return (f32x4_t){kk < dim ? r[kk] : 0.f, kk + 1 < dim ? r[kk + 1] : 0.f, kk + 2 < dim ? r[kk + 2] : 0.f,
                   kk + 3 < dim ? r[kk + 3] : 0.f};
}

inline size_t vs_scan_lds_bytes(bool topk, uint32_t cap) {
  return (size_t)(kVsTileDocs + kVsTileQ) * kVsRow * 4 + kVsTileDocs * 8 + (topk ? (size_t)kVsTileQ * cap * 8 : 0);
}

// ---- the epilogue of a scan tile, shared by vs_scan_kernel, the bf16 first pass of the two-pass search
//      (slg_vsearch_approx.hpp) and the IVF scan (slg_vsearch_ivf.hpp): all three leave the scores of a 64 x 128
//      tile in the C/D layout of the 16x16 MFMAs ----
// what a lane carries from tile to tile: its query (16w + qc of the workgroup's 64), the query's boost and
// filter, and (top-k form) the entries its query's LDS buffer holds and the threshold key
struct VsEpilogue {
  uint32_t lane, w, qc, g;
  uint32_t myq;
  float bst;
  int32_t flt;
  uint32_t cap;
  uint64_t *s_buf, *my_buf;   // [64][cap] of the workgroup; this lane's query's row
  uint32_t cnt, th_hi, th_lo;
};
// is (seg, doc) deleted, or rejected by filter flt (< 0: none)?  Keeps the lane's reject bitmap of the segment at hand
struct VsReject {
  const uint32_t *rej = nullptr;
  uint32_t rej_seg = 0xFFFFFFFFu;
  bool rej_all = false;
  __device__ __forceinline__ bool operator()(const VsScanParams &p, const int32_t flt, uint32_t seg, uint32_t doc) {
    if (seg != rej_seg) {
      rej_seg = seg;
      rej_all = false;
      if (flt < 0) {
        rej = p.segs[seg].deleted;
      } else if ((uint32_t)flt < p.n_filters) {
        rej = p.reject_table[(size_t)flt * p.n_segs + seg];
        rej_all = rej == nullptr;  // (a filter without a bitmap for this segment matches nothing)
      } else {
        rej = nullptr;
        rej_all = true;  // (no such filter: matches nothing)
      }
    }
    return rej_all || (rej && ((rej[doc >> 5] >> (doc & 31)) & 1u));
  }
};
// the fused top-k epilogue of one tile of 128 docs: sim(acc[ti][r], i) is the similarity of this lane's query and
// doc i = 16 ti + 4 g + r of the tile (s_seg[i] = its segment or ~0: no vector, s_doc[i] = the doc in it, flat(i) =
// its flat id: base + i in the scans of the flat space, a table in the IVF scan).  Times the boost it becomes a
// key, and the keys that beat the threshold go to the query's buffer.
// (The store form stays inline in each scan kernel: as a function it costs vs_scan_kernel<1, false> two more
// AGPR copies.)
template <typename Flat, typename Sim>
__device__ __forceinline__ void vs_tile_topk(const VsScanParams &p, VsEpilogue &e, Flat &&flat,
                                             const uint32_t *s_seg, const uint32_t *s_doc, const f32x4_t (&acc)[8],
                                             Sim &&sim) {
  const uint32_t lane = e.lane, w = e.w, qc = e.qc, g = e.g, cap = e.cap;
  const bool q_ok = e.myq < p.nq;
  const int32_t flt = e.flt;
  const float bst = e.bst;
  uint32_t cnt = e.cnt, th_hi = e.th_hi, th_lo = e.th_lo;
  VsReject rejected;
#pragma unroll
  for (int ti = 0; ti < 8; ti++) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const uint32_t i = 16 * ti + 4 * g + r;
      float s = sim(acc[ti][r], i);
      s = s * bst;
      const uint32_t seg = s_seg[i];
      const uint32_t hi = ordered_score(s), lo = ~flat(i);
      auto beats = [&]() { return hi > th_hi || (hi == th_hi && lo > th_lo); };
      bool pass = q_ok && seg != 0xFFFFFFFFu && beats();
      if (__ballot(pass) == 0ull) continue;
      pass = pass && !rejected(p, flt, seg, s_doc[i]);
      // room for 4 more entries of every query of this wave
      uint64_t need = __ballot(g == 0 && cnt + 4 > cap);
      while (need) {
        const uint32_t j = (uint32_t)__builtin_ctzll(need);
        need &= need - 1;
        const uint32_t n = rl(cnt, j);
        uint64_t *b = e.s_buf + (size_t)(16 * w + j) * cap;
        const uint32_t kept = vs_compact(b, n, p.k, lane);
        if (qc == j) {
          cnt = kept;
          if (n >= p.k) {
            const uint64_t kth = b[p.k - 1];
            th_hi = (uint32_t)(kth >> 32);
            th_lo = (uint32_t)kth;
          }
        }
      }
      pass = pass && beats();
      const uint64_t m = __ballot(pass);
      const uint32_t b0 = (uint32_t)(m >> qc) & 1u, b1 = (uint32_t)(m >> (16 + qc)) & 1u,
                     b2 = (uint32_t)(m >> (32 + qc)) & 1u, b3 = (uint32_t)(m >> (48 + qc)) & 1u;
      const uint32_t pre = (g > 0 ? b0 : 0u) + (g > 1 ? b1 : 0u) + (g > 2 ? b2 : 0u);
      wave_fence();
      if (pass) e.my_buf[cnt + pre] = ((uint64_t)hi << 32) | lo;
      wave_fence();
      cnt += b0 + b1 + b2 + b3;
    }
  }
  e.cnt = cnt;
  e.th_hi = th_hi;
  e.th_lo = th_lo;
}

// (top-k form, after the last tile) the partial list of each query of the wave: its k best, sorted, at slot *o of
// p.out, as slot(j, &o) says for the wave's query j: write it, skip this query, or stop (no later query has a slot).
// The scans of the flat space write the slot of (query, chunk), the IVF scan that of (query, probe rank, chunk)
enum VsSlot { kVsSlotWrite, kVsSlotSkip, kVsSlotStop };
template <typename Slot>
__device__ __forceinline__ void vs_write_partials(const VsScanParams &p, const VsEpilogue &e, Slot &&slot) {
  for (uint32_t j = 0; j < 16; j++) {
    size_t o = 0;
    const VsSlot s = slot(j, &o);
    if (s == kVsSlotStop) break;
    if (s == kVsSlotSkip) continue;
    uint64_t *b = e.s_buf + (size_t)(16 * e.w + j) * e.cap;
    const uint32_t kept = vs_compact(b, rl(e.cnt, j), p.k, e.lane);
    p.out[o * kVsSmallK + e.lane] = e.lane < kept ? b[e.lane] : 0ull;
  }
}

// ---- the f32 tile body, shared by vs_scan_kernel and the cosine IVF scan (slg_vsearch_ivf.hpp): the raw scores of the
//      workgroup's 64 queries (rows qrow, null = none) x 128 docs (rows drow) into acc, through the LDS tiles sA
//      [128][kVsRow] / sB [64][kVsRow], kVsKc dimensions at a time, the next step's rows in flight under this one's
//      products.  METRIC 0: dot products on the matrix cores; 1: sum (q - x)^2 on the VALU.  The order of the
//      floating-point operations is part of the result: both searches return the same bits ----
template <int METRIC>
__device__ __forceinline__ void vs_tile_scores(float *sA, float *sB, const float *(&drow)[4],
                                               const float *(&qrow)[2], const uint32_t dim, const bool vec4,
                                               const bool qvec4, f32x4_t (&acc)[8]) {
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t qc = lane & 15u, g = lane >> 4;
  const uint32_t col = 4 * (t & 7u);
#pragma unroll
  for (int i = 0; i < 8; i++) acc[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  f32x4_t ra[4], rb[2];
#pragma unroll
  for (int i = 0; i < 4; i++) ra[i] = vs_ld4(drow[i], col, dim, vec4);
#pragma unroll
  for (int j = 0; j < 2; j++) rb[j] = vs_ld4(qrow[j], col, dim, qvec4);
  for (uint32_t k0 = 0; k0 < dim; k0 += kVsKc) {
    __syncthreads();  // the previous step's reads are done
#pragma unroll
    for (int i = 0; i < 4; i++) *reinterpret_cast<f32x4_t *>(sA + ((t >> 3) + 32 * i) * kVsRow + col) = ra[i];
#pragma unroll
    for (int j = 0; j < 2; j++) *reinterpret_cast<f32x4_t *>(sB + ((t >> 3) + 32 * j) * kVsRow + col) = rb[j];
    __syncthreads();
    if (k0 + kVsKc < dim) {  // the next step's rows, in flight under this step's products
#pragma unroll
      for (int i = 0; i < 4; i++) ra[i] = vs_ld4(drow[i], k0 + kVsKc + col, dim, vec4);
#pragma unroll
      for (int j = 0; j < 2; j++) rb[j] = vs_ld4(qrow[j], k0 + kVsKc + col, dim, qvec4);
    }
    if (METRIC == 0) {
      // lane group g feeds k = 4g + c of each 16-wide half (component c = one MFMA): the same k
      // permutation on both operands
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const f32x4_t b = *reinterpret_cast<const f32x4_t *>(sB + (16 * w + qc) * kVsRow + 16 * h + 4 * g);
#pragma unroll
        for (int ti = 0; ti < 8; ti++) {
          const f32x4_t a = *reinterpret_cast<const f32x4_t *>(sA + (16 * ti + qc) * kVsRow + 16 * h + 4 * g);
          acc[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[ti], 0, 0, 0);
          acc[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[ti], 0, 0, 0);
          acc[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[ti], 0, 0, 0);
          acc[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[ti], 0, 0, 0);
        }
      }
    } else {
      for (uint32_t kk = 0; kk < kVsKc; kk += 4) {
        const f32x4_t b = *reinterpret_cast<const f32x4_t *>(sB + (16 * w + qc) * kVsRow + kk);
#pragma unroll
        for (int ti = 0; ti < 8; ti++) {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const f32x4_t a = *reinterpret_cast<const f32x4_t *>(sA + (16 * ti + 4 * g + r) * kVsRow + kk);
            const float d0 = b.x - a.x, d1 = b.y - a.y, d2 = b.z - a.z, d3 = b.w - a.w;
            float s = acc[ti][r];
            s += d0 * d0;
            s += d1 * d1;
            s += d2 * d2;
            s += d3 * d3;
            acc[ti][r] = s;
          }
        }
      }
    }
  }
}
// metric_similarity (vectors/mod.rs:107-120) of a raw score of vs_tile_scores
template <int METRIC>
struct VsExactSim {
  __device__ __forceinline__ float operator()(float s, uint32_t) const {
    return METRIC == 0 ? (s != s ? 0.0f : s) : -sqrtf(s);
  }
};

// METRIC 0: cosine on the matrix cores; 1: L2 on the VALU.  TOPK: fused top-k (else: store keys).
// Lane l of wave w holds, per tile t of 16 docs, the scores of query 16w + (l & 15) and docs
// 16t + 4(l >> 4) + r, r < 4 (the D layout of v_mfma_f32_16x16x4_f32 with A = docs, B = queries).
template <int METRIC, bool TOPK>
__global__ void __launch_bounds__(256) vs_scan_kernel(VsScanParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *sA = reinterpret_cast<float *>(smem);          // [128][kVsRow] docs
  float *sB = sA + kVsTileDocs * kVsRow;                // [64][kVsRow] queries
  uint32_t *s_seg = reinterpret_cast<uint32_t *>(sB + kVsTileQ * kVsRow);  // [128] segment or ~0 (no vector)
  uint32_t *s_doc = s_seg + kVsTileDocs;                // [128] doc in its segment
  uint64_t *s_buf = reinterpret_cast<uint64_t *>(s_doc + kVsTileDocs);    // [64][cap] (TOPK)
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t qc = lane & 15u, g = lane >> 4;
  const uint32_t q0 = blockIdx.x * kVsTileQ;
  const uint32_t dim = p.dim;
  const bool vec4 = (dim & 3u) == 0;
  // this lane's query in the epilogue
  const uint32_t myq = q0 + 16 * w + qc;
  const bool q_ok = myq < p.nq;
  const float bst = q_ok && p.boost ? p.boost[(size_t)myq * p.n_clauses + p.clause] : 1.0f;
  const int32_t flt = q_ok && p.q_filter ? p.q_filter[myq] : -1;
  const uint32_t cap = p.cap;
  VsEpilogue e{lane, w, qc, g, myq, bst, flt, cap, s_buf, s_buf + (size_t)(16 * w + qc) * cap, 0, 0, 0};
  // this thread's query rows for the staging loads: rows (t >> 3) + 32 j
  const float *qrow[2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const uint32_t q = q0 + (t >> 3) + 32 * j;
    qrow[j] = q < p.nq ? p.qvecs + (size_t)q * p.q_stride + p.q_off : nullptr;
  }
  const uint32_t total = p.doc_base[p.n_segs];

  const uint32_t tb = p.tile_begin + blockIdx.y * p.tiles_per_block;
  uint32_t te = tb + p.tiles_per_block;
  te = te < p.tile_end ? te : p.tile_end;
  for (uint32_t tile = tb; tile < te; tile++) {
    const uint32_t base = tile * kVsTileDocs;
    const float *drow[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t r = (t >> 3) + 32 * i, flat = base + r;
      drow[i] = nullptr;
      uint32_t seg = 0xFFFFFFFFu, doc = 0;
      if (flat < total) {
        const uint32_t s = vs_seg_of(p.doc_base, p.n_segs, flat);
        const VecSegDev vd = p.vsegs[s];
        doc = flat - p.doc_base[s];
        if (vd.dim == dim && doc < vd.n_docs) {
          const uint32_t off = vd.offsets[doc];
          if (off != 0xFFFFFFFFu) {
            drow[i] = vd.values + (size_t)off * dim;
            seg = s;
          }
        }
      }
      if ((t & 7u) == 0) {
        s_seg[r] = seg;
        s_doc[r] = doc;
      }
    }
    f32x4_t acc[8];
    vs_tile_scores<METRIC>(sA, sB, drow, qrow, dim, vec4, vec4 && p.qvec4, acc);
    // ---- epilogue: metric_similarity (vectors/mod.rs:107-120), * boost (api/reader.rs:2421) ----
    const VsExactSim<METRIC> sim;
    if constexpr (TOPK) {
      vs_tile_topk(p, e, [&](uint32_t i) { return base + i; }, s_seg, s_doc, acc, sim);
    } else {
      VsReject rejected;
#pragma unroll
      for (int ti = 0; ti < 8; ti++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const uint32_t i = 16 * ti + 4 * g + r;
          const float s = sim(acc[ti][r], i) * bst;
          const uint32_t seg = s_seg[i];
          const uint32_t hi = ordered_score(s), lo = ~(base + i);
          const bool ok = q_ok && seg != 0xFFFFFFFFu && !rejected(p, flt, seg, s_doc[i]);
          if (q_ok) p.out[(size_t)myq * p.out_stride + (base + i - p.tile_begin * kVsTileDocs)] =
              ok ? (((uint64_t)hi << 32) | lo) : 0ull;
        }
      }
    }
    __syncthreads();  // s_seg / s_doc of the next tile
  }
  if (!TOPK) return;
  vs_write_partials(p, e, [&](uint32_t j, size_t *o) {
    const uint32_t q = q0 + 16 * w + j;
    *o = (size_t)q * p.n_chunks + blockIdx.y;
    return q < p.nq ? kVsSlotWrite : kVsSlotStop;
  });
}

// block-wide bitonic sort, descending, of P (a power of two) keys at a (LDS or global memory)
template <typename T>
__device__ __forceinline__ void vs_bitonic_desc(T *a, uint32_t P) {
  for (uint32_t size = 2; size <= P; size <<= 1)
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t i = threadIdx.x; i < P / 2; i += blockDim.x) {
        const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const T x = a[lo], y = a[hi];
        const bool desc = (lo & size) == 0;
        if (desc ? x < y : x > y) {
          a[lo] = y;
          a[hi] = x;
        }
      }
      __syncthreads();
    }
}

__host__ __device__ inline uint32_t vs_pow2(uint32_t n) {
  uint32_t P = 1;
  while (P < n) P <<= 1;
  return P;
}

// fold n_in candidate keys of (clause c, query q) into the query's running top-k of the clause;
// final: also leave the list sorted by doc in dlist as (flat << 32 | score bits)
struct VsSelectParams {
  const uint64_t *in;  // (blockIdx.y * nq + q) * in_stride
  uint32_t n_in, in_stride;
  uint64_t *run;       // [clause][q][k] best first
  uint32_t *run_cnt;   // [clause][q]
  uint64_t *dlist;     // [clause][q][k]
  uint32_t nq, k, c0, final_;
  // hybrid search (slg_hybrid.hpp: the keys hy_gather_kernel appended): the workgroups are queries q0 + x;
  // query q's keys of clause c0 + y start at in + y * in_stride + (in_off[q] - in_base), in_cnt[clause][q] of
  // them, and this pass folds those from in_skip on, at most n_in.  in_off == nullptr: the layout above
  const uint64_t *in_off;
  const uint32_t *in_cnt;
  uint64_t in_base;
  uint32_t in_skip, q0;
};

__global__ void __launch_bounds__(kVsSortThreads) vs_select_kernel(VsSelectParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t *s = reinterpret_cast<uint64_t *>(smem);
  __shared__ uint32_t s_n;
  const uint32_t q = p.q0 + blockIdx.x, c = p.c0 + blockIdx.y;
  const size_t qc = (size_t)c * p.nq + q;
  const uint64_t *in = p.in + ((size_t)blockIdx.y * p.nq + q) * p.in_stride;
  uint32_t n_in = p.n_in;
  if (p.in_off) {
    const uint32_t have = p.in_cnt[qc];
    n_in = have > p.in_skip ? (have - p.in_skip < n_in ? have - p.in_skip : n_in) : 0u;
    in = p.in + (size_t)blockIdx.y * p.in_stride + (p.in_off[q] - p.in_base) + p.in_skip;
    if (n_in == 0 && !p.final_) return;  // (nothing of this query in this pass)
  }
  uint64_t *run = p.run + qc * p.k;
  const uint32_t cnt = p.run_cnt[qc];
  const uint64_t th = cnt >= p.k ? run[p.k - 1] : 0ull;
  for (uint32_t i = threadIdx.x; i < cnt; i += blockDim.x) s[i] = run[i];
  if (threadIdx.x == 0) s_n = cnt;
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n_in; i += blockDim.x) {
    const uint64_t key = in[i];
    if (key > th) s[atomicAdd(&s_n, 1u)] = key;
  }
  __syncthreads();
  const uint32_t n = s_n, P = vs_pow2(n);
  for (uint32_t i = n + threadIdx.x; i < P; i += blockDim.x) s[i] = 0ull;
  __syncthreads();
  vs_bitonic_desc(s, P);
  const uint32_t m = n < p.k ? n : p.k;
  for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) run[i] = s[i];
  if (threadIdx.x == 0) p.run_cnt[qc] = m;
  if (!p.final_) return;
  const uint32_t Pm = vs_pow2(m);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < Pm; i += blockDim.x) {
    const uint64_t key = i < m ? s[i] : 0ull;  // (descending sort of the complement = ascending flat)
    s[i] = i < m ? ~(((uint64_t)~(uint32_t)key << 32) | (uint32_t)__float_as_int(vs_key_score(key))) : 0ull;
  }
  __syncthreads();
  vs_bitonic_desc(s, Pm);
  uint64_t *dl = p.dlist + qc * p.k;
  for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) dl[i] = ~s[i];
}

// ---- union of the clause lists + compute_hybrid_score at bm25 = 0 (api/reader.rs:225-254) + the
//      top k_out by (final desc, segment asc, doc asc) ----
struct VsBlendParams {
  const uint64_t *dlist;
  const uint32_t *run_cnt;
  uint32_t nq, k, n_clauses;
  const float *alpha;  // [nq][n_clauses]
  int32_t metric[8];
  const uint32_t *doc_base;
  uint32_t n_segs;
  uint64_t *ukeys;  // [nq][P] when P > kVsSortCap (else LDS)
  uint32_t P, k_out;
  uint32_t *out_doc, *out_seg;
  float *out_score, *out_vec;
  uint32_t *out_count;
  uint64_t *out_total;
  // (HYBRID) the BM25 hits of the batch: rows [nq][bm_k], bm_count[q] of them filled; Pb = vs_pow2(bm_k) keys
  // of work space per query: behind the union keys in LDS (bm_lds), else at bkeys
  const uint32_t *bm_doc, *bm_seg;
  const float *bm_score;
  const uint32_t *bm_count;
  uint64_t *bkeys;
  uint32_t bm_k, Pb, bm_lds;
};

// HYBRID (merge_vector_hits, api/reader.rs:2474-2537): the union also holds the query's BM25 hits, a union
// doc's bm25 is its score among those hits or 0.0 (:2496-2500), and when every alpha is <= 0 a doc that no
// clause list holds is dropped (all_vector_only, :2494,2504); such a row's vector score, the reference's None,
// is the missing-vector score of clause 0's metric, as the rerank kernels write it.
template <bool HYBRID>
__global__ void __launch_bounds__(kVsSortThreads) vs_blend_kernel(VsBlendParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ uint32_t s_n;
  const uint32_t q = blockIdx.x, NC = p.n_clauses;
  uint64_t *u = p.P > kVsSortCap ? p.ukeys + (size_t)q * p.P : reinterpret_cast<uint64_t *>(smem);
  // (HYBRID) the BM25 hits as (flat << 32 | score bits), descending, so by flat doc for the binary search
  const uint64_t *bl = nullptr;
  uint32_t nb = 0;
  bool vec_only = false;
  if constexpr (HYBRID) {
    uint64_t *b = p.bm_lds ? reinterpret_cast<uint64_t *>(smem) + p.P : p.bkeys + (size_t)q * p.Pb;
    nb = p.bm_count[q] < p.bm_k ? p.bm_count[q] : p.bm_k;
    for (uint32_t i = threadIdx.x; i < p.Pb; i += blockDim.x) {
      uint64_t key = 0ull;
      if (i < nb) {
        const size_t o = (size_t)q * p.bm_k + i;
        const uint32_t sg = p.bm_seg[o] < p.n_segs ? p.bm_seg[o] : 0u;
        key = ((uint64_t)(p.doc_base[sg] + p.bm_doc[o]) << 32) | (uint32_t)__float_as_int(p.bm_score[o]);
      }
      b[i] = key;
    }
    __syncthreads();
    vs_bitonic_desc(b, p.Pb);
    __syncthreads();
    bl = b;
    vec_only = true;
    for (uint32_t cc = 0; cc < NC; cc++) vec_only = vec_only && p.alpha[(size_t)q * NC + cc] <= 0.0f;
  }
  // (HYBRID) the BM25 score of flat, if it is a BM25 hit
  auto bm_lookup = [&](uint32_t flat, float *bm) -> bool {
    uint32_t lo = 0, hi = nb;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      const uint32_t f = (uint32_t)(bl[mid] >> 32);
      if (f == flat) {
        *bm = __int_as_float((int32_t)(uint32_t)bl[mid]);
        return true;
      }
      if (f > flat)
        lo = mid + 1;
      else
        hi = mid;
    }
    return false;
  };
  auto list = [&](uint32_t c) { return p.dlist + ((size_t)c * p.nq + q) * p.k; };
  auto count = [&](uint32_t c) { return p.run_cnt[(size_t)c * p.nq + q]; };
  // the score of flat in clause c's list, if it is there
  auto lookup = [&](uint32_t c, uint32_t flat, float *vs) -> bool {
    const uint64_t *l = list(c);
    uint32_t lo = 0, hi = count(c);
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      const uint32_t f = (uint32_t)(l[mid] >> 32);
      if (f == flat) {
        *vs = __int_as_float((int32_t)(uint32_t)l[mid]);
        return true;
      }
      if (f < flat)
        lo = mid + 1;
      else
        hi = mid;
    }
    return false;
  };
  // compute_hybrid_score, clauses in order: the final score and the vector sum
  auto hybrid = [&](uint32_t flat, float *vsum, bool *has) -> float {
    float bm = 0.0f;
    if constexpr (HYBRID) (void)bm_lookup(flat, &bm);
    float blended_sum = 0.0f, vector_sum = 0.0f;
    bool found = false;
    for (uint32_t cc = 0; cc < NC; cc++) {
      float vs;
      if (lookup(cc, flat, &vs)) {
        vector_sum += vs;
        found = true;
      } else {
        vs = missing_vector_score(p.metric[cc]);  // (:217-223)
      }
      blended_sum += blend(p.alpha[(size_t)q * NC + cc], bm, vs);
    }
    *vsum = vector_sum;
    *has = found;
    return blended_sum / (float)NC;
  };
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  if constexpr (HYBRID) {
    for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) {
      const uint32_t flat = (uint32_t)(bl[i] >> 32);
      float vsum;
      bool has;
      const float fin = hybrid(flat, &vsum, &has);
      if (vec_only && !has) continue;
      u[atomicAdd(&s_n, 1u)] = ((uint64_t)ordered_score(fin) << 32) | (uint32_t)~flat;
    }
  }
  for (uint32_t c = 0; c < NC; c++) {
    const uint64_t *l = list(c);
    const uint32_t n = count(c);
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      const uint32_t flat = (uint32_t)(l[i] >> 32);
      bool seen = false;  // a doc belongs to the first clause whose list holds it
      float dummy;
      if constexpr (HYBRID) seen = bm_lookup(flat, &dummy);  // (or to the BM25 hits)
      for (uint32_t cc = 0; cc < c && !seen; cc++) seen = lookup(cc, flat, &dummy);
      if (seen) continue;
      float vsum;
      bool has;
      const float fin = hybrid(flat, &vsum, &has);
      u[atomicAdd(&s_n, 1u)] = ((uint64_t)ordered_score(fin) << 32) | (uint32_t)~flat;
    }
  }
  __syncthreads();
  const uint32_t U = s_n, P = vs_pow2(U);
  for (uint32_t i = U + threadIdx.x; i < P; i += blockDim.x) u[i] = 0ull;
  __syncthreads();
  vs_bitonic_desc(u, P);
  for (uint32_t i = threadIdx.x; i < p.k_out; i += blockDim.x) {
    const size_t o = (size_t)q * p.k_out + i;
    if (i < U) {
      const uint64_t key = u[i];
      const uint32_t flat = ~(uint32_t)key;
      const uint32_t seg = vs_seg_of(p.doc_base, p.n_segs, flat);
      float vsum;
      bool has;
      (void)hybrid(flat, &vsum, &has);
      p.out_doc[o] = flat - p.doc_base[seg];
      p.out_seg[o] = seg;
      p.out_score[o] = vs_key_score(key);
      if (p.out_vec) p.out_vec[o] = HYBRID && !has ? missing_vector_score(p.metric[0]) : vsum;
    } else {
      p.out_doc[o] = 0u;
      p.out_seg[o] = 0u;
      p.out_score[o] = 0.0f;
      if (p.out_vec) p.out_vec[o] = 0.0f;
    }
  }
  if (threadIdx.x == 0) {
    p.out_count[q] = U < p.k_out ? U : p.k_out;
    p.out_total[q] = U;
  }
}

}  // namespace slg
