// slg_vsearch_train.hpp — Lloyd steps over the f32 store of a vector field (slg_index_train_vector_field): the kernels
// of the centroid update.  Assignment and list build are slg_index_cluster_vector_field's own (slg_vsearch_ivf.hpp).
//
//   one step: the rows are assigned to the centroids C_{t-1} and the lists are built (docs ascending inside a list);
//     vs_ivf_moved_kernel counts the rows whose list changed; vs_ivf_sum_kernel takes, per (list, chunk of
//     kIvfTrainChunk docs) item, the f64 sum of the chunk's rows in doc order; vs_ivf_centroid_kernel adds a list's
//     chunk sums in chunk order, forms the mean and the new centroid, or keeps the previous one.
//   every floating-point addition has a fixed place in a fixed order: no floating-point atomics, and the result does
//     not depend on how the items are spread over the workgroups.
#pragma once

#include "slg_vsearch_ivf.hpp"

namespace slg {

constexpr uint32_t kIvfTrainChunk = 256;    // docs of one partial sum (SLG_VECTOR_TRAIN_CHUNK)
constexpr uint32_t kIvfTrainThreads = 256;  // dim d belongs to thread d mod 256
constexpr uint32_t kIvfTrainPasses = 4;     // dims of one thread summed side by side (a group of 1024 dims)
constexpr uint32_t kIvfTrainUnroll = 8;     // rows whose loads are issued together
constexpr uint32_t kIvfTrainTile = 2048;    // dims of one LDS tile of the mean in vs_ivf_centroid_kernel

// ---- the start: centroid i = row floor(i * n_rows / n_lists) of the store, as stored ----
struct IvfStartParams {
  const float *values;  // [n_rows][dim]
  float *centroids;     // [n_lists][dim]
  uint32_t n_rows, n_lists, dim;
};
__global__ void __launch_bounds__(256) vs_ivf_start_kernel(IvfStartParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)p.n_lists * p.dim) return;
  const uint64_t l = i / p.dim, d = i % p.dim;
  const uint64_t row = l * (uint64_t)p.n_rows / p.n_lists;
  if (row < p.n_rows) p.centroids[i] = p.values[row * p.dim + d];
}

// ---- the rows whose list differs from the previous assignment's (integer atomics: the sum has no order) ----
struct IvfMovedParams {
  const uint32_t *row_list, *prev;  // [n_rows]
  uint32_t n_rows;
  uint32_t *moved;                  // zeroed by the caller
};
__global__ void __launch_bounds__(256) vs_ivf_moved_kernel(IvfMovedParams p) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool diff = r < p.n_rows && p.row_list[r] != p.prev[r];
  const uint64_t m = __ballot(diff);
  if ((threadIdx.x & 63u) == 0 && m) atomicAdd(p.moved, (uint32_t)__popcll(m));
}

// ---- the partial sums: one workgroup per (list, chunk) item ----
struct IvfSumItem {
  uint32_t d_begin, d_end;  // a range of the lists' doc array, at most kIvfTrainChunk docs of one list
};
struct IvfSumParams {
  const IvfSumItem *items;  // [n_items]
  const uint32_t *docs;     // the lists' docs
  const uint32_t *offsets;  // [n_docs] row or 0xFFFFFFFF
  const float *values;      // [n_rows][dim]
  double *partial;          // [n_items][dim]
  uint32_t n_items, n_docs, n_rows, dim;
};
// NP x 256 dims from d0 on, this thread's NP of them side by side.  Every load is unconditional (a dim past the end
// reads the row's last one, a doc without a row reads row 0, and the value is replaced by +0.0, which changes no sum
// that started from +0.0), so the loads of kIvfTrainUnroll rows are issued together; only the additions are ordered.
template <uint32_t NP>
__device__ __forceinline__ void ivf_sum_group(const IvfSumParams &p, const uint32_t *s_row, uint32_t n, uint32_t d0,
                                              uint32_t it) {
  const uint32_t t = threadIdx.x, dim = p.dim;
  uint32_t dc[NP];
#pragma unroll
  for (uint32_t j = 0; j < NP; j++) {
    const uint32_t d = d0 + j * kIvfTrainThreads + t;
    dc[j] = d < dim ? d : dim - 1;
  }
  double acc[NP];
#pragma unroll
  for (uint32_t j = 0; j < NP; j++) acc[j] = 0.0;
  uint32_t i = 0;
  for (; i + kIvfTrainUnroll <= n; i += kIvfTrainUnroll) {
    float v[kIvfTrainUnroll][NP];
#pragma unroll
    for (uint32_t u = 0; u < kIvfTrainUnroll; u++) {
      const uint32_t row = s_row[i + u];
      const bool ok = row != 0xFFFFFFFFu;
      const float *src = p.values + (size_t)(ok ? row : 0u) * dim;
#pragma unroll
      for (uint32_t j = 0; j < NP; j++) {
        const float x = src[dc[j]];
        v[u][j] = ok ? x : 0.0f;
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < kIvfTrainUnroll; u++) {
#pragma unroll
      for (uint32_t j = 0; j < NP; j++) acc[j] += (double)v[u][j];
    }
  }
  for (; i < n; i++) {
    const uint32_t row = s_row[i];
    const bool ok = row != 0xFFFFFFFFu;
    const float *src = p.values + (size_t)(ok ? row : 0u) * dim;
    float v[NP];
#pragma unroll
    for (uint32_t j = 0; j < NP; j++) {
      const float x = src[dc[j]];
      v[j] = ok ? x : 0.0f;
    }
#pragma unroll
    for (uint32_t j = 0; j < NP; j++) acc[j] += (double)v[j];
  }
#pragma unroll
  for (uint32_t j = 0; j < NP; j++) {
    const uint32_t d = d0 + j * kIvfTrainThreads + t;
    if (d < dim) p.partial[(size_t)it * dim + d] = acc[j];
  }
}
__global__ void __launch_bounds__(kIvfTrainThreads) vs_ivf_sum_kernel(IvfSumParams p) {
  __shared__ uint32_t s_row[kIvfTrainChunk];  // the rows of the item's docs, in doc order (0xFFFFFFFF: none)
  const uint32_t t = threadIdx.x, dim = p.dim;
  if (dim == 0 || p.n_rows == 0) return;
  for (uint32_t it = blockIdx.x; it < p.n_items; it += gridDim.x) {
    const IvfSumItem item = p.items[it];
    const uint32_t n = item.d_end - item.d_begin < kIvfTrainChunk ? item.d_end - item.d_begin : kIvfTrainChunk;
    __syncthreads();  // (s_row of the previous item)
    if (t < kIvfTrainChunk) {
      uint32_t row = 0xFFFFFFFFu;
      if (t < n) {
        const uint32_t doc = p.docs[item.d_begin + t];
        if (doc < p.n_docs) row = p.offsets[doc];
        if (row >= p.n_rows) row = 0xFFFFFFFFu;
      }
      s_row[t] = row;
    }
    __syncthreads();
    for (uint32_t d0 = 0; d0 < dim; d0 += kIvfTrainThreads * kIvfTrainPasses) {
      const uint32_t np = (dim - d0 + kIvfTrainThreads - 1) / kIvfTrainThreads;
      if (np >= 4)
        ivf_sum_group<4>(p, s_row, n, d0, it);
      else if (np == 3)
        ivf_sum_group<3>(p, s_row, n, d0, it);
      else if (np == 2)
        ivf_sum_group<2>(p, s_row, n, d0, it);
      else
        ivf_sum_group<1>(p, s_row, n, d0, it);
    }
  }
}

// ---- the new centroids: one workgroup per list ----
struct IvfCentroidParams {
  const double *partial;       // [n_items][dim]
  const uint32_t *item_begin;  // [n_lists + 1] first item of each list
  const uint32_t *list_begin;  // [n_lists + 1]
  const float *prev;           // [n_lists][dim] C_{t-1}
  float *next;                 // [n_lists][dim] C_t
  uint32_t n_lists, dim;
  int32_t metric;
};
__global__ void __launch_bounds__(kIvfTrainThreads) vs_ivf_centroid_kernel(IvfCentroidParams p) {
  __shared__ float s_m[kIvfTrainTile];
  __shared__ double s_s;
  const uint32_t l = blockIdx.x, t = threadIdx.x, dim = p.dim;
  if (l >= p.n_lists) return;
  const uint32_t n = p.list_begin[l + 1] - p.list_begin[l];
  const uint32_t c0 = p.item_begin[l], c1 = p.item_begin[l + 1];
  const float *prev = p.prev + (size_t)l * dim;
  float *next = p.next + (size_t)l * dim;
  if (n == 0) {  // an empty list keeps its centroid
    for (uint32_t d = t; d < dim; d += kIvfTrainThreads) next[d] = prev[d];
    return;
  }
  const double dn = (double)n;
  double s = 0.0;  // (thread 0's)
  for (uint32_t d0 = 0; d0 < dim; d0 += kIvfTrainTile) {
    const uint32_t d1 = d0 + kIvfTrainTile < dim ? d0 + kIvfTrainTile : dim;
    __syncthreads();  // (s_m of the previous tile is read)
    for (uint32_t d = d0 + t; d < d1; d += kIvfTrainThreads) {
      double sum = 0.0;
      for (uint32_t c = c0; c < c1; c++) sum += p.partial[(size_t)c * dim + d];
      const float m = (float)__ddiv_rn(sum, dn);
      s_m[d - d0] = m;
      next[d] = m;  // (read again below by this same thread)
    }
    __syncthreads();
    if (t == 0)
      for (uint32_t d = d0; d < d1; d++) {
        const double m = (double)s_m[d - d0];
        s += m * m;
      }
  }
  if (t == 0) s_s = s;
  __syncthreads();
  s = s_s;
  const bool finite = s - s == 0.0;  // neither NaN nor an infinity
  const bool adopt = finite && (p.metric != 0 || s > 0.0);
  if (!adopt) {
    for (uint32_t d = t; d < dim; d += kIvfTrainThreads) next[d] = prev[d];
  } else if (p.metric == 0) {
    const double norm = __dsqrt_rn(s);
    for (uint32_t d = t; d < dim; d += kIvfTrainThreads) next[d] = (float)__ddiv_rn((double)next[d], norm);
  }
}

}  // namespace slg
