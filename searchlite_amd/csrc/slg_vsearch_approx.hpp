// slg_vsearch_approx.hpp — two-pass vector search (slg_vector_search_batch_approx*): a first pass over a bf16
// copy of the store picks `refine` candidates per (clause, query), a second pass scores them again from the f32
// store in the exact scan's own arithmetic, and the select / blend tail of slg_vsearch.hpp runs unchanged.
//
//   vs_quantize_kernel    the copy (slg_index_quantize_vector_field): every f32 row rounded to bf16 (nearest even;
//                         NaN stays NaN, +-inf stays, denormals round like any value), padded with zeros to a
//                         multiple of kVaKc, and the row's f32 squared norm, summed left to right
//   vs_scan_bf16_kernel   the roles of vs_scan_kernel over the copy: tiles of 64 queries x 128 docs, products on
//                         v_mfma_f32_16x16x32_bf16 (f32 accumulation), queries rounded to bf16 as they are staged.
//                         Cosine: the dot (NaN -> 0); L2: -sqrt(max(0, |x|^2 + |q|^2 - 2 x.q)) from the stored f32
//                         norm and the f32 norm of the f32 query (the cancellation that rules this form out of the
//                         exact scan only moves a doc across the refine boundary here).  The accumulators have the
//                         C/D layout of the exact scan's, so the top-k epilogue is vs_tile_topk itself
//   vs_refine_kernel      every key of every list scored again: cosine through v_mfma_f32_16x16x4_f32 with the
//                         operand feed of vs_scan_kernel (k0 step, 16-wide half, component, lane group), so the
//                         score is the exact scan's bit for bit; L2 the left-to-right sum of (q - x)^2
#pragma once

#include "slg_vsearch.hpp"

namespace slg {

constexpr uint32_t kVaKc = 64;  // bf16 dimensions staged per step: one 128-byte LDS row (+ 16 bytes = kVsRow floats)

__host__ __device__ inline uint32_t va_dim_pad(uint32_t dim) { return (dim + kVaKc - 1) / kVaKc * kVaKc; }

// f32 -> bf16, round to nearest even
__device__ __forceinline__ uint32_t va_bf16(float x) {
  const uint32_t b = (uint32_t)__float_as_int(x);
  if (x != x) return (b >> 16) | 0x40u;  // (a NaN whose payload sits in the low half would round to inf)
  return (b + 0x7FFFu + ((b >> 16) & 1u)) >> 16;
}

struct VsQuantParams {
  const float *values;  // [n_rows * dim]
  uint16_t *rows;       // [n_rows * dim_pad]
  float *norms;         // [n_rows]
  uint32_t n_rows, dim, dim_pad;
};

// one wave per row
__global__ void __launch_bounds__(256) vs_quantize_kernel(VsQuantParams p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t step = gridDim.x * 4u;
  for (uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6); row < p.n_rows; row += step) {
    const float *src = p.values + (size_t)row * p.dim;
    uint16_t *dst = p.rows + (size_t)row * p.dim_pad;
    for (uint32_t k = lane; k < p.dim_pad; k += 64u) dst[k] = k < p.dim ? (uint16_t)va_bf16(src[k]) : (uint16_t)0;
    if (lane == 0) {
      float s = 0.0f;
      for (uint32_t k = 0; k < p.dim; k++) s += src[k] * src[k];
      p.norms[row] = s;
    }
    if (row + step < row) break;  // (2^32 - 1 rows at most)
  }
}

struct VsScanBf16Params {
  VsScanParams s;           // as vs_scan_kernel's (vsegs: offsets and dim; values are not read)
  const VecCopyDev *csegs;  // the clause field's per-segment copies
};

inline size_t va_scan_lds_bytes(bool topk, uint32_t cap) { return vs_scan_lds_bytes(topk, cap) + kVsTileDocs * 4; }

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// Lane l of wave w holds, per tile t of 16 docs, the scores of query 16w + (l & 15) and docs 16t + 4(l >> 4) + r:
// the D layout of v_mfma_f32_16x16x32_bf16 with A = docs, B = queries, the exact scan's.  Its A / B fragment is 8
// consecutive k of one row, k = 8(l >> 4) + j: one 16-byte LDS read.  LDS rows are 144 bytes (64 bf16 + 16), which
// spreads the 16 rows of a 16-byte read over all banks.
template <int METRIC, bool TOPK>
__global__ void __launch_bounds__(256) vs_scan_bf16_kernel(VsScanBf16Params pp) {
  const VsScanParams &p = pp.s;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr uint32_t kRowB = kVsRow * 4;                         // bytes of an LDS row
  unsigned char *sA = smem;                                      // [128][kRowB] docs
  unsigned char *sB = sA + kVsTileDocs * kRowB;                  // [64][kRowB] queries
  uint32_t *s_seg = reinterpret_cast<uint32_t *>(sB + kVsTileQ * kRowB);  // [128] segment or ~0 (no vector)
  uint32_t *s_doc = s_seg + kVsTileDocs;                         // [128] doc in its segment
  float *s_nrm = reinterpret_cast<float *>(s_doc + kVsTileDocs);  // [128] |x|^2 (L2)
  uint64_t *s_buf = reinterpret_cast<uint64_t *>(s_nrm + kVsTileDocs);   // [64][cap] (TOPK)
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t qc = lane & 15u, g = lane >> 4;
  const uint32_t q0 = blockIdx.x * kVsTileQ;
  const uint32_t dim = p.dim;
  const bool vec4 = (dim & 3u) == 0 && p.qvec4;
  // this lane's query in the epilogue
  const uint32_t myq = q0 + 16 * w + qc;
  const bool q_ok = myq < p.nq;
  const float bst = q_ok && p.boost ? p.boost[(size_t)myq * p.n_clauses + p.clause] : 1.0f;
  const int32_t flt = q_ok && p.q_filter ? p.q_filter[myq] : -1;
  const uint32_t cap = p.cap;
  VsEpilogue e{lane, w, qc, g, myq, bst, flt, cap, s_buf, s_buf + (size_t)(16 * w + qc) * cap, 0, 0, 0};
  float qn = 0.0f;  // (L2) |q|^2 of the f32 query
  if (METRIC == 1 && q_ok) {
    const float *qv = p.qvecs + (size_t)myq * p.q_stride + p.q_off;
    for (uint32_t k = 0; k < dim; k++) qn += qv[k] * qv[k];
  }
  // this thread's query rows for the staging loads: rows (t >> 3) + 32 j, 8 dimensions from col
  const float *qrow[2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const uint32_t q = q0 + (t >> 3) + 32 * j;
    qrow[j] = q < p.nq ? p.qvecs + (size_t)q * p.q_stride + p.q_off : nullptr;
  }
  const uint32_t col = 8 * (t & 7u);
  const uint32_t total = p.doc_base[p.n_segs];
  const uint32_t dim_pad = va_dim_pad(dim);
  const u32x4_t z4 = {0u, 0u, 0u, 0u};
  auto ld_doc = [&](const uint16_t *row, uint32_t kk) -> u32x4_t {
    typedef const __attribute__((address_space(1))) u32x4_t *gv_t;
    return row ? *(gv_t)(row + kk) : z4;  // (rows are padded to dim_pad: no bound on kk < dim_pad)
  };
  auto pack_q = [&](const f32x4_t lo, const f32x4_t hi) -> u32x4_t {
    return (u32x4_t){va_bf16(lo.x) | (va_bf16(lo.y) << 16), va_bf16(lo.z) | (va_bf16(lo.w) << 16),
                     va_bf16(hi.x) | (va_bf16(hi.y) << 16), va_bf16(hi.z) | (va_bf16(hi.w) << 16)};
  };

  const uint32_t tb = p.tile_begin + blockIdx.y * p.tiles_per_block;
  uint32_t te = tb + p.tiles_per_block;
  te = te < p.tile_end ? te : p.tile_end;
  for (uint32_t tile = tb; tile < te; tile++) {
    const uint32_t base = tile * kVsTileDocs;
    const uint16_t *drow[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t r = (t >> 3) + 32 * i, flat = base + r;
      drow[i] = nullptr;
      uint32_t seg = 0xFFFFFFFFu, doc = 0;
      float nrm = 0.0f;
      if (flat < total) {
        const uint32_t s = vs_seg_of(p.doc_base, p.n_segs, flat);
        const VecSegDev vd = p.vsegs[s];
        const VecCopyDev cd = pp.csegs[s];
        doc = flat - p.doc_base[s];
        if (vd.dim == dim && cd.rows && cd.dim_pad == dim_pad && doc < vd.n_docs) {
          const uint32_t off = vd.offsets[doc];
          if (off != 0xFFFFFFFFu) {
            drow[i] = cd.rows + (size_t)off * dim_pad;
            if (METRIC == 1) nrm = cd.norms[off];
            seg = s;
          }
        }
      }
      if ((t & 7u) == 0) {
        s_seg[r] = seg;
        s_doc[r] = doc;
        if (METRIC == 1) s_nrm[r] = nrm;
      }
    }
    f32x4_t acc[8];
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    u32x4_t ra[4];
    f32x4_t rb[2][2];
#pragma unroll
    for (int i = 0; i < 4; i++) ra[i] = ld_doc(drow[i], col);
#pragma unroll
    for (int j = 0; j < 2; j++) {
      rb[j][0] = vs_ld4(qrow[j], col, dim, vec4);
      rb[j][1] = vs_ld4(qrow[j], col + 4, dim, vec4);
    }
    for (uint32_t k0 = 0; k0 < dim_pad; k0 += kVaKc) {
      __syncthreads();  // the previous step's reads are done
#pragma unroll
      for (int i = 0; i < 4; i++) *reinterpret_cast<u32x4_t *>(sA + ((t >> 3) + 32 * i) * kRowB + 2 * col) = ra[i];
#pragma unroll
      for (int j = 0; j < 2; j++)
        *reinterpret_cast<u32x4_t *>(sB + ((t >> 3) + 32 * j) * kRowB + 2 * col) = pack_q(rb[j][0], rb[j][1]);
      __syncthreads();
      if (k0 + kVaKc < dim_pad) {  // the next step's rows, in flight under this step's products
#pragma unroll
        for (int i = 0; i < 4; i++) ra[i] = ld_doc(drow[i], k0 + kVaKc + col);
#pragma unroll
        for (int j = 0; j < 2; j++) {
          rb[j][0] = vs_ld4(qrow[j], k0 + kVaKc + col, dim, vec4);
          rb[j][1] = vs_ld4(qrow[j], k0 + kVaKc + col + 4, dim, vec4);
        }
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {  // two MFMA k-steps of 32: lane group g feeds k = 32h + 8g .. + 7
        const bf16x8_t b = *reinterpret_cast<const bf16x8_t *>(sB + (16 * w + qc) * kRowB + 64 * h + 16 * g);
#pragma unroll
        for (int ti = 0; ti < 8; ti++) {
          const bf16x8_t a = *reinterpret_cast<const bf16x8_t *>(sA + (16 * ti + qc) * kRowB + 64 * h + 16 * g);
          acc[ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[ti], 0, 0, 0);
        }
      }
    }
    // ---- epilogue: the first-pass similarity, * boost ----
    const auto sim = [&](float s, uint32_t i) {
      if (METRIC == 0) return s != s ? 0.0f : s;
      return -sqrtf(fmaxf((s_nrm[i] + qn) - 2.0f * s, 0.0f));
    };
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
    __syncthreads();  // s_seg / s_doc / s_nrm of the next tile
  }
  if (!TOPK) return;
  vs_write_partials(p, e, [&](uint32_t j, size_t *o) {
    const uint32_t q = q0 + 16 * w + j;
    *o = (size_t)q * p.n_chunks + blockIdx.y;
    return q < p.nq ? kVsSlotWrite : kVsSlotStop;
  });
}

// ---- pass 2: the exact score of every first-pass candidate ----
struct VsRefineParams {
  const VecSegDev *vsegs;
  const uint32_t *doc_base;
  uint32_t n_segs, dim, nq;
  const float *qvecs;
  uint32_t q_stride, q_off, qvec4;
  const float *boost;  // [nq][n_clauses] or nullptr
  uint32_t n_clauses, clause;
  uint64_t *run;            // [clause][nq][k]: the first pass's keys, best first; rewritten in place
  const uint32_t *run_cnt;  // [clause][nq] keys held; the slots behind them are zeroed here
  uint32_t k;
};

// the f32 row of a key's doc (null: the doc has no vector in the field, which the first pass never returns)
__device__ __forceinline__ const float *va_key_row(const VsRefineParams &p, uint64_t key) {
  if (key == 0ull) return nullptr;
  const uint32_t flat = ~(uint32_t)key;
  const uint32_t s = vs_seg_of(p.doc_base, p.n_segs, flat);
  const VecSegDev vd = p.vsegs[s];
  const uint32_t doc = flat - p.doc_base[s];
  if (vd.dim != p.dim || doc >= vd.n_docs) return nullptr;
  const uint32_t off = vd.offsets[doc];
  return off != 0xFFFFFFFFu ? vd.values + (size_t)off * p.dim : nullptr;
}

// One workgroup per query.  Cosine: a wave scores 16 candidates at a time as the A rows of v_mfma_f32_16x16x4_f32
// against the query in every B column, with vs_scan_kernel's feed: per 32-dimension step and 16-wide half, lane group
// g supplies dimensions 4g + c, component c = one MFMA, zeros past dim.  L2: a lane per candidate.
template <int METRIC>
__global__ void __launch_bounds__(256) vs_refine_kernel(VsRefineParams p) {
  const uint32_t q = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const size_t lq = (size_t)p.clause * p.nq + q;
  uint64_t *list = p.run + lq * p.k;
  const uint32_t n = p.run_cnt[lq];
  const float *qv = p.qvecs + (size_t)q * p.q_stride + p.q_off;
  const float bst = p.boost ? p.boost[(size_t)q * p.n_clauses + p.clause] : 1.0f;
  const uint32_t dim = p.dim;
  if (METRIC == 0) {
    const bool vec4 = (dim & 3u) == 0;
    const uint32_t qc = lane & 15u, g = lane >> 4;
    for (uint32_t c0 = 16 * w; c0 < p.k; c0 += 64) {
      const uint32_t i = c0 + qc;
      const float *row = va_key_row(p, i < n ? list[i] : 0ull);
      uint64_t mine[4];  // the keys of the rows this lane writes: candidates c0 + 4g + r
#pragma unroll
      for (int r = 0; r < 4; r++) mine[r] = c0 + 4 * g + r < n ? list[c0 + 4 * g + r] : 0ull;
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
      for (uint32_t k0 = 0; k0 < dim; k0 += kVsKc) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const f32x4_t a = vs_ld4(row, k0 + 16 * h + 4 * g, dim, vec4);
          const f32x4_t b = vs_ld4(qv, k0 + 16 * h + 4 * g, dim, vec4 && p.qvec4);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
        }
      }
      if (qc == 0) {  // (every column holds the query: column 0 writes)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const uint32_t o = c0 + 4 * g + r;
          if (o >= p.k) continue;
          float s = acc[r];
          s = s != s ? 0.0f : s;
          s = s * bst;
          list[o] = mine[r] ? (((uint64_t)ordered_score(s) << 32) | (uint32_t)mine[r]) : 0ull;
        }
      }
    }
  } else {
    for (uint32_t i = t; i < p.k; i += blockDim.x) {
      const uint64_t key = i < n ? list[i] : 0ull;
      const float *row = va_key_row(p, key);
      float s = 0.0f;
      if (row)
        for (uint32_t kk = 0; kk < dim; kk++) {
          const float d = qv[kk] - row[kk];
          s += d * d;
        }
      s = -sqrtf(s);
      s = s * bst;
      list[i] = key ? (((uint64_t)ordered_score(s) << 32) | (uint32_t)key) : 0ull;
    }
  }
}

}  // namespace slg
