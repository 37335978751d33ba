// slg_vsearch_ivf.hpp — vector search over an inverted-file index of a vector field (slg_index_cluster_vector_field,
// slg_vector_search_batch_ivf*): the docs of a segment are grouped into lists around caller-supplied centroids, and
// a query scores only the docs of its `nprobe` nearest lists, from the f32 store, in vs_scan_kernel's arithmetic.
//
//   building the lists: the rows of a store are the queries and the centroids the docs of an exact scan with a
//     top-1 (vs_scan_kernel over a pseudo-segment; the products commute, so the chain is the exact call's).  Then
//     count per (list, doc range), prefix per list, exclusive scan of the list lengths, and a fill in which one wave
//     walks each doc range in order: docs ascend inside a list, and nothing depends on the order atomics land in.
//   searching: (1) the coarse step is the exact scan over the centroid tables as pseudo-segments and
//     vs_select_kernel's top nprobe; (2) the probes are inverted into per-list query groups (count, exclusive scan,
//     fill) and a work table of (list, 64 of its queries, chunk of its docs) items; (3) vs_ivf_scan_kernel walks the
//     table and leaves one partial top-k list per (query, probe rank, chunk); vs_select_kernel folds them.
//     The scan owns how an item finds its queries and docs; the tile body (vs_tile_scores; the L2 form keeps a copy
//     of the L2 body, which is faster there) and the top-k epilogue (vs_tile_topk, vs_write_partials) are the exact
//     scan's functions.
#pragma once

#include "slg_vsearch.hpp"

namespace slg {

constexpr uint32_t kIvfScanThreads = 1024;   // the single-block exclusive scans
constexpr uint32_t kIvfRangeDocs = 4096;     // docs of a fill range (a wave each), at least
constexpr uint32_t kIvfMaxRanges = 256;
constexpr uint32_t kIvfListChunks = 4;       // doc chunks of the longest list, at most
// (kIvfUnclChunks, slg_desc.hpp: doc chunks of an unclustered segment, at most)

// ---- block-wide exclusive scan of one value per thread (kIvfScanThreads threads); *total = the sum ----
__device__ __forceinline__ uint32_t ivf_block_excl(uint32_t v, uint32_t *s, uint32_t *total) {
  const uint32_t t = threadIdx.x;
  __syncthreads();  // (s of the previous call)
  s[t] = v;
  __syncthreads();
  for (uint32_t off = 1; off < kIvfScanThreads; off <<= 1) {
    const uint32_t x = t >= off ? s[t - off] : 0u;
    __syncthreads();
    s[t] += x;
    __syncthreads();
  }
  *total = s[kIvfScanThreads - 1];
  return s[t] - v;
}

// ---- building the lists ----
// the list of each row of a batch: the best key of its partial lists (vs_scan_kernel<., true> with k = 1 over the
// centroids as docs: key order = score desc, list asc)
struct IvfBestParams {
  const uint64_t *partials;  // [(row * n_chunks + chunk) * kVsSmallK]
  uint32_t n_rows, n_chunks;
  uint32_t *row_list;        // [n_rows] of the batch
};
__global__ void __launch_bounds__(256) vs_ivf_best_kernel(IvfBestParams p) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.n_rows) return;
  uint64_t best = 0ull;
  for (uint32_t c = 0; c < p.n_chunks; c++) {
    const uint64_t k = p.partials[((size_t)r * p.n_chunks + c) * kVsSmallK];
    best = k > best ? k : best;
  }
  p.row_list[r] = ~(uint32_t)best;
}

struct IvfBuildParams {
  const uint32_t *offsets;   // [n_docs] row or 0xFFFFFFFF
  const uint32_t *row_list;  // [n_rows]
  uint32_t *doc_list;        // [n_docs] list or 0xFFFFFFFF
  uint32_t *table;           // [n_lists][n_ranges] docs of (list, range); then the prefix inside the list
  uint32_t *lens;            // [n_lists]
  uint32_t *list_begin;      // [n_lists + 1]
  uint32_t *docs;            // the lists' docs
  uint32_t n_docs, n_lists, n_ranges, range_docs;
};
__global__ void __launch_bounds__(256) vs_ivf_count_kernel(IvfBuildParams p) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= p.n_docs) return;
  const uint32_t off = p.offsets[d];
  uint32_t l = 0xFFFFFFFFu;
  if (off != 0xFFFFFFFFu) {
    l = p.row_list[off];
    if (l >= p.n_lists) l = 0xFFFFFFFFu;
  }
  p.doc_list[d] = l;
  if (l != 0xFFFFFFFFu) atomicAdd(&p.table[(size_t)l * p.n_ranges + d / p.range_docs], 1u);
}
__global__ void __launch_bounds__(256) vs_ivf_prefix_kernel(IvfBuildParams p) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= p.n_lists) return;
  uint32_t run = 0;
  for (uint32_t r = 0; r < p.n_ranges; r++) {
    const uint32_t x = p.table[(size_t)l * p.n_ranges + r];
    p.table[(size_t)l * p.n_ranges + r] = run;
    run += x;
  }
  p.lens[l] = run;
}
// exclusive scan of n values into out[0 .. n] (one workgroup)
struct IvfScanParams {
  const uint32_t *in;
  uint32_t *out;
  uint32_t n;
};
__global__ void __launch_bounds__(kIvfScanThreads) vs_ivf_exscan_kernel(IvfScanParams p) {
  __shared__ uint32_t s[kIvfScanThreads];
  uint32_t base = 0;
  for (uint32_t i0 = 0; i0 < p.n; i0 += kIvfScanThreads) {
    const uint32_t i = i0 + threadIdx.x;
    uint32_t total;
    const uint32_t e = ivf_block_excl(i < p.n ? p.in[i] : 0u, s, &total);
    if (i < p.n) p.out[i] = base + e;
    base += total;
  }
  if (threadIdx.x == 0) p.out[p.n] = base;
}
// one wave per doc range, docs in order: a doc's place is its list's begin + the list's docs of earlier ranges +
// those of this range before it
__global__ void __launch_bounds__(64) vs_ivf_fill_kernel(IvfBuildParams p) {
  const uint32_t r = blockIdx.x, lane = threadIdx.x;
  const uint32_t d0 = r * p.range_docs;
  uint32_t d1 = d0 + p.range_docs;
  d1 = d1 < p.n_docs ? d1 : p.n_docs;
  for (uint32_t d = d0; d < d1; d += 64) {
    const uint32_t doc = d + lane;
    const uint32_t l = doc < d1 ? p.doc_list[doc] : 0xFFFFFFFFu;
    uint32_t rank = 0, same = 0, leader = 64;
    for (uint32_t j = 0; j < 64; j++) {
      const uint32_t lj = rl(l, j);
      if (lj == l) {
        leader = leader == 64 ? j : leader;
        rank += j < lane ? 1u : 0u;
        same++;
      }
    }
    uint32_t base = 0;
    if (l != 0xFFFFFFFFu && lane == leader) base = atomicAdd(&p.table[(size_t)l * p.n_ranges + r], same);
    base = (uint32_t)__shfl((int)base, (int)(leader & 63u));
    if (l != 0xFFFFFFFFu) p.docs[p.list_begin[l] + base + rank] = doc;
  }
}

// ---- searching: the probes inverted into per-list query groups and a work table ----
// (IvfUncl, slg_desc.hpp: an unclustered segment of the field, a list behind the field's own that holds all queries)
// one item of the work table: up to 64 queries of a list's group x a chunk of the list's docs
struct IvfItem {
  uint32_t seg;
  uint32_t d_begin, d_end;  // a range of the segment's list docs array (uncl: of its doc ids)
  uint32_t g_begin, g_n;    // the queries: pairs[g_begin ..] (uncl: queries g_begin ..), g_n <= 64 of them
  uint32_t slot;            // added to the pair's slot: the chunk (uncl: the segment's slot + the chunk)
  uint32_t uncl, pad;
};
struct IvfPlanParams {
  const uint64_t *probes;      // [nq][n_probe] the coarse step's keys, best first: (ordered key << 32) | ~list
  const VecListDev *lsegs;     // [n_segs]
  const uint32_t *list_base;   // [n_segs + 1] first flat list of each segment
  const IvfUncl *uncl;         // [n_uncl]
  uint32_t n_segs, n_lists, n_uncl, nq, n_probe;
  uint32_t list_chunk_docs, list_chunks;  // docs of a list chunk; chunks of the longest list
  uint32_t *cnt;               // [n_lists] queries of each list              | zeroed at the start of the call
  uint32_t *cursor;            // [n_lists] pairs filled                       |
  uint32_t *goff;              // [n_lists + n_uncl + 1] first pair of each list's group
  uint32_t *ioff;              // [n_lists + n_uncl + 1] first item of each list
  uint32_t *n_items;
  uint2 *pairs;                // (query, first partial slot of the probe rank)
  IvfItem *items;
  uint32_t items_cap;
};
__device__ __forceinline__ uint32_t ivf_list_len(const IvfPlanParams &p, uint32_t L, uint32_t *seg, uint32_t *begin) {
  const uint32_t s = vs_seg_of(p.list_base, p.n_segs, L);
  const VecListDev ld = p.lsegs[s];
  const uint32_t l = L - p.list_base[s];
  *seg = s;
  if (!ld.list_begin || l >= ld.n_lists) {
    *begin = 0;
    return 0;
  }
  *begin = ld.list_begin[l];
  return ld.list_begin[l + 1] - ld.list_begin[l];
}
__global__ void __launch_bounds__(256) vs_ivf_probe_count_kernel(IvfPlanParams p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.nq * p.n_probe) return;
  const uint64_t key = p.probes[i];
  const uint32_t L = ~(uint32_t)key;
  if (key != 0ull && L < p.n_lists) atomicAdd(&p.cnt[L], 1u);
}
// (one workgroup) the groups' and the items' first positions, and the item count
__global__ void __launch_bounds__(kIvfScanThreads) vs_ivf_plan_kernel(IvfPlanParams p) {
  __shared__ uint32_t s[kIvfScanThreads];
  const uint32_t n = p.n_lists + p.n_uncl, qtiles = (p.nq + kVsTileQ - 1) / kVsTileQ;
  uint32_t gbase = 0, ibase = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += kIvfScanThreads) {
    const uint32_t L = i0 + threadIdx.x;
    uint32_t c = 0, items = 0;
    if (L < p.n_lists) {
      uint32_t seg, begin;
      const uint32_t len = ivf_list_len(p, L, &seg, &begin);
      c = p.cnt[L];
      items = ((c + kVsTileQ - 1) / kVsTileQ) * ((len + p.list_chunk_docs - 1) / p.list_chunk_docs);
    } else if (L < n) {
      const IvfUncl u = p.uncl[L - p.n_lists];
      items = qtiles * ((u.n_docs + u.chunk_docs - 1) / u.chunk_docs);
    }
    uint32_t total;
    const uint32_t ge = ivf_block_excl(c, s, &total);
    if (L < n) p.goff[L] = gbase + ge;
    gbase += total;
    const uint32_t ie = ivf_block_excl(items, s, &total);
    if (L < n) p.ioff[L] = ibase + ie;
    ibase += total;
  }
  if (threadIdx.x == 0) {
    p.goff[n] = gbase;
    p.ioff[n] = ibase;
    *p.n_items = ibase < p.items_cap ? ibase : p.items_cap;
  }
}
// the items of one list at items[at .. end): tiles of 64 of its n_queries queries (from g0) x chunks of chunk_docs of
// its len docs (from begin of the segment's array); an item's slot = slot0 + its chunk
__device__ __forceinline__ void ivf_emit_items(const IvfPlanParams &p, uint32_t at, const uint32_t end, uint32_t seg,
                                               uint32_t begin, uint32_t len, uint32_t chunk_docs, uint32_t g0,
                                               uint32_t n_queries, uint32_t slot0, uint32_t uncl) {
  for (uint32_t q0 = 0; q0 < n_queries; q0 += kVsTileQ)
    for (uint32_t d = 0, ch = 0; d < len; d += chunk_docs, ch++) {
      if (at >= end) return;
      const uint32_t de = d + chunk_docs < len ? d + chunk_docs : len;
      p.items[at++] = IvfItem{seg, begin + d, begin + de, g0 + q0, n_queries - q0 < kVsTileQ ? n_queries - q0 : kVsTileQ,
                              slot0 + ch, uncl, 0u};
    }
}
// thread i: pair i = (query, probe rank) goes to its list's group; list i's items go to the work table
__global__ void __launch_bounds__(256) vs_ivf_items_kernel(IvfPlanParams p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < p.nq * p.n_probe) {
    const uint64_t key = p.probes[i];
    const uint32_t L = ~(uint32_t)key;
    if (key != 0ull && L < p.n_lists) {
      const uint32_t pos = p.goff[L] + atomicAdd(&p.cursor[L], 1u);
      p.pairs[pos] = make_uint2(i / p.n_probe, (i % p.n_probe) * p.list_chunks);
    }
  }
  const uint32_t n = p.n_lists + p.n_uncl;
  if (i >= n) return;
  uint32_t at = p.ioff[i];
  const uint32_t end = p.ioff[i + 1] < p.items_cap ? p.ioff[i + 1] : p.items_cap;
  if (i < p.n_lists) {
    uint32_t seg, begin;
    const uint32_t len = ivf_list_len(p, i, &seg, &begin);
    ivf_emit_items(p, at, end, seg, begin, len, p.list_chunk_docs, p.goff[i], p.cnt[i], 0u, 0u);
  } else {
    const IvfUncl u = p.uncl[i - p.n_lists];
    ivf_emit_items(p, at, end, u.seg, 0u, u.n_docs, u.chunk_docs, 0u, p.nq, p.n_probe * p.list_chunks + u.slot, 1u);
  }
}

// ---- the scan of the work table ----
struct VsIvfScanParams {
  VsScanParams s;  // the exact scan's: stores, tombstones, filters, queries, boost; out = the partial lists
                   // [(q * slots_q + slot) * kVsSmallK]; tile_* / n_chunks / out_stride unused
  const VecListDev *lsegs;
  const IvfItem *items;
  const uint32_t *n_items;
  const uint2 *pairs;
  uint32_t slots_q;  // partial slots of a query
};

inline size_t vs_ivf_scan_lds_bytes(uint32_t cap) {
  return vs_scan_lds_bytes(true, cap) + kVsTileDocs * 4 + kVsTileQ * 8;
}

// vs_scan_kernel's tile over the docs of a list and the queries of its group: the tile body is vs_tile_scores (cosine)
// and the epilogue vs_tile_topk / vs_write_partials (slg_vsearch.hpp), with the docs' flat ids from a table and one
// VsEpilogue per item.  TOPK: the only form built.
template <int METRIC, bool TOPK>
__global__ void __launch_bounds__(256) vs_ivf_scan_kernel(VsIvfScanParams ip) {
  static_assert(TOPK, "the store form of the IVF scan is not built");
  const VsScanParams &p = ip.s;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *sA = reinterpret_cast<float *>(smem);          // [128][kVsRow] docs
  float *sB = sA + kVsTileDocs * kVsRow;                // [64][kVsRow] queries
  uint32_t *s_seg = reinterpret_cast<uint32_t *>(sB + kVsTileQ * kVsRow);  // [128] segment or ~0 (no vector)
  uint32_t *s_doc = s_seg + kVsTileDocs;                // [128] doc in its segment
  uint64_t *s_buf = reinterpret_cast<uint64_t *>(s_doc + kVsTileDocs);    // [64][cap]
  uint32_t *s_flat = reinterpret_cast<uint32_t *>(s_buf + (size_t)kVsTileQ * p.cap);  // [128] flat doc
  uint32_t *s_q = s_flat + kVsTileDocs;                 // [64] query or ~0
  uint32_t *s_slot = s_q + kVsTileQ;                    // [64] the query's partial slot of this item
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t qc = lane & 15u, g = lane >> 4;
  const uint32_t dim = p.dim, cap = p.cap;
  const bool vec4 = (dim & 3u) == 0;
  const uint32_t n_items = *ip.n_items;

  for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const IvfItem item = ip.items[it];
    __syncthreads();  // the previous item's partials are written
    if (t < kVsTileQ) {
      uint32_t q = 0xFFFFFFFFu, slot = item.slot;
      if (t < item.g_n) {
        if (item.uncl) {
          q = item.g_begin + t;
        } else {
          const uint2 pr = ip.pairs[item.g_begin + t];
          q = pr.x;
          slot += pr.y;
        }
        if (q >= p.nq) q = 0xFFFFFFFFu;
      }
      s_q[t] = q;
      s_slot[t] = slot;
    }
    __syncthreads();
    // this lane's query in the epilogue (~0, which no nq exceeds: none)
    const uint32_t myq = s_q[16 * w + qc];
    const bool q_ok = myq != 0xFFFFFFFFu;
    const float bst = q_ok && p.boost ? p.boost[(size_t)myq * p.n_clauses + p.clause] : 1.0f;
    const int32_t flt = q_ok && p.q_filter ? p.q_filter[myq] : -1;
    VsEpilogue e{lane, w, qc, g, myq, bst, flt, cap, s_buf, s_buf + (size_t)(16 * w + qc) * cap, 0, 0, 0};
    const float *qrow[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const uint32_t q = s_q[(t >> 3) + 32 * j];
      qrow[j] = q != 0xFFFFFFFFu ? p.qvecs + (size_t)q * p.q_stride + p.q_off : nullptr;
    }
    const VecSegDev vd = p.vsegs[item.seg];
    const uint32_t *ldocs = item.uncl ? nullptr : ip.lsegs[item.seg].docs;
    const uint32_t seg_base = p.doc_base[item.seg];

    for (uint32_t base = item.d_begin; base < item.d_end; base += kVsTileDocs) {
      const float *drow[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t r = (t >> 3) + 32 * i, at = base + r;
        drow[i] = nullptr;
        uint32_t seg = 0xFFFFFFFFu, doc = 0;
        if (at < item.d_end) {
          doc = ldocs ? ldocs[at] : at;
          if (vd.dim == dim && doc < vd.n_docs) {
            const uint32_t off = vd.offsets[doc];
            if (off != 0xFFFFFFFFu) {
              drow[i] = vd.values + (size_t)off * dim;
              seg = item.seg;
            }
          }
        }
        if ((t & 7u) == 0) {
          s_seg[r] = seg;
          s_doc[r] = doc;
          s_flat[r] = seg_base + doc;
        }
      }
      f32x4_t acc[8];
      if constexpr (METRIC == 0) {
        vs_tile_scores<0>(sA, sB, drow, qrow, dim, vec4, vec4 && p.qvec4, acc);
      } else {
        // the L2 tile body of vs_tile_scores, written out: through the function this kernel takes 165 registers
        // for 284 and, on the one workgroup per CU its grid has, the call at nprobe 1 / 64 took 7.623 / 19.109 ms
        // for 6.326 / 16.126 (profiles/vsearch_fold_time.txt)
        const uint32_t col = 4 * (t & 7u);
#pragma unroll
        for (int i = 0; i < 8; i++) acc[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        f32x4_t ra[4], rb[2];
#pragma unroll
        for (int i = 0; i < 4; i++) ra[i] = vs_ld4(drow[i], col, dim, vec4);
#pragma unroll
        for (int j = 0; j < 2; j++) rb[j] = vs_ld4(qrow[j], col, dim, vec4 && p.qvec4);
        for (uint32_t k0 = 0; k0 < dim; k0 += kVsKc) {
          __syncthreads();  // the previous step's reads are done
#pragma unroll
          for (int i = 0; i < 4; i++) *reinterpret_cast<f32x4_t *>(sA + ((t >> 3) + 32 * i) * kVsRow + col) = ra[i];
#pragma unroll
          for (int j = 0; j < 2; j++) *reinterpret_cast<f32x4_t *>(sB + ((t >> 3) + 32 * j) * kVsRow + col) = rb[j];
          __syncthreads();
          if (k0 + kVsKc < dim) {  // the next step's rows, in flight under this step's sums
#pragma unroll
            for (int i = 0; i < 4; i++) ra[i] = vs_ld4(drow[i], k0 + kVsKc + col, dim, vec4);
#pragma unroll
            for (int j = 0; j < 2; j++) rb[j] = vs_ld4(qrow[j], k0 + kVsKc + col, dim, vec4 && p.qvec4);
          }
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
      vs_tile_topk(p, e, [&](uint32_t i) { return s_flat[i]; }, s_seg, s_doc, acc, VsExactSim<METRIC>());
      __syncthreads();  // s_seg / s_doc / s_flat of the next tile
    }
    // the item's partial list of each of its queries, in the slot of (query, probe rank, chunk)
    vs_write_partials(p, e, [&](uint32_t j, size_t *o) {
      const uint32_t q = s_q[16 * w + j], slot = s_slot[16 * w + j];
      *o = (size_t)q * ip.slots_q + slot;
      return q != 0xFFFFFFFFu && slot < ip.slots_q ? kVsSlotWrite : kVsSlotSkip;
    });
  }
}

}  // namespace slg
