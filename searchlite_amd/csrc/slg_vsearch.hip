// slg_vsearch.hip — exact vector-only search (slg_vector_search_batch*; kernels: slg_vsearch.hpp) and the two-pass
// search over a bf16 copy of the store (slg_vector_search_batch_approx*; kernels: slg_vsearch_approx.hpp) and the
// search over the inverted-file lists of a field (slg_vector_search_batch_ivf*; kernels: slg_vsearch_ivf.hpp).
#include "slg_host.hpp"

#include "slg_vsearch.hpp"
#include "slg_vsearch_approx.hpp"
#include "slg_vsearch_ivf.hpp"
#include "slg_vsearch_train.hpp"

using namespace slghost;

static_assert(slg::kIvfTrainChunk == SLG_VECTOR_TRAIN_CHUNK, "the chunk of a partial sum is part of the ABI");

bool slghost::vs_prepare(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                         uint32_t cand_size, uint32_t k_out, const VsArgs &a, bool host_filter, VsCall *vc,
                         std::shared_ptr<const IndexState> state) {
  SLG_REQUIRE(ix != nullptr && clause_field != nullptr, "index or clause_field is NULL");
  if (n_clauses < 1 || n_clauses > SLG_MAX_VECTOR_CLAUSES)
    throw SlgError(SLG_ERR_UNSUPPORTED, "n_clauses outside 1..SLG_MAX_VECTOR_CLAUSES");
  if (cand_size < 1 || cand_size > SLG_MAX_VECTOR_CANDIDATES)
    throw SlgError(SLG_ERR_UNSUPPORTED, "cand_size outside 1..SLG_MAX_VECTOR_CANDIDATES");
  if (k_out > SLG_MAX_K) throw SlgError(SLG_ERR_UNSUPPORTED, "k_out > SLG_MAX_K");
  if (nq == 0) return false;
  SLG_REQUIRE(a.qvecs && a.alpha && a.out_count && a.out_total, "query or count arrays are NULL");
  SLG_REQUIRE(k_out == 0 || (a.out_doc && a.out_seg && a.out_score), "output arrays are NULL");
  vc->S = state ? state : ix->snapshot();
  const IndexState &S = *vc->S;
  SLG_REQUIRE(S.total_docs < 0xFFFFFFFFull, "more than 2^32 - 2 docs in the index");
  vc->nq = nq;
  vc->n_clauses = n_clauses;
  vc->cand = cand_size;
  vc->k_out = k_out;
  for (uint32_t c = 0; c < n_clauses; c++) {
    field_facts(S, clause_field[c], &vc->dim[c], &vc->metric[c], &vc->vsegs[c]);
    vc->coff[c] = vc->q_floats;
    vc->q_floats += vc->dim[c];
  }
  if (host_filter && a.q_filter)
    for (uint32_t q = 0; q < nq; q++) {
      const int32_t f = a.q_filter[q];
      if (f < 0) continue;
      SLG_REQUIRE(S.filter_usable((size_t)f), "q_filter names no filter registered for every segment");
    }
  return true;
}

std::shared_ptr<VecCopySeg> slghost::vs_quantize_store(slg_index *ix, const float *d_values, uint32_t n_rows,
                                                       uint32_t dim) {
  auto c = std::make_shared<VecCopySeg>();
  c->n_rows = n_rows;
  c->dim = dim;
  c->dim_pad = slg::va_dim_pad(dim);
  c->rows.alloc((size_t)n_rows * c->dim_pad * 2, &ix->pool);
  c->norms.alloc((size_t)n_rows * 4, &ix->pool);
  if (n_rows) {
    slg::VsQuantParams qp{d_values, c->rows.as<uint16_t>(), c->norms.as<float>(), n_rows, dim, c->dim_pad};
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n_rows + 3) / 4, 1u << 20);
    hipLaunchKernelGGL(slg::vs_quantize_kernel, dim3(blocks), dim3(256), 0, ix->stream, qp);
    SLG_HIP(hipGetLastError());
    SLG_HIP(hipStreamSynchronize(ix->stream));
  }
  return c;
}

namespace {
// workgroups of one round of a scan with lds bytes of LDS each: as many as the LDS of a CU holds, at most by_vgprs
// (3: the VGPR bound of vs_scan_kernel)
uint32_t vs_resident_groups(slg_index *ix, size_t lds, uint32_t by_vgprs = 3u) {
  int n_cu = 0;
  SLG_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ix->device));
  const uint32_t per_cu = std::min<uint32_t>(by_vgprs, (uint32_t)((160u << 10) / lds));
  return std::max<uint32_t>((uint32_t)n_cu, 1u) * std::max<uint32_t>(per_cu, 1u);
}

// the doc chunks of a top-k scan whose workgroups (qtiles x chunks) fill one round of `target` resident ones: at
// most max_chunks (1 .. n_tiles), each of tpb of the n_tiles tiles
struct VsChunks {
  uint32_t n_chunks, tpb;
};
VsChunks vs_round_chunks(uint32_t target, uint32_t qtiles, uint32_t n_tiles, uint32_t max_chunks) {
  const uint32_t want = std::max<uint32_t>((target + qtiles - 1) / qtiles, 1u);
  const uint32_t n = std::min<uint32_t>(want, max_chunks);
  const uint32_t tpb = (n_tiles + n - 1) / n;
  return VsChunks{(n_tiles + tpb - 1) / tpb, tpb};
}

// are 16-byte loads of clause c's query vectors aligned?
uint32_t vs_qvec4(const VsCall &vc, const VsArgs &a, uint32_t c) {
  return (vc.q_floats % 4 == 0 && vc.coff[c] % 4 == 0 && ((uintptr_t)a.qvecs & 15) == 0) ? 1u : 0u;
}

// what every scan of clause c of a call shares: the index's stores, tombstones and filters (a scan over
// pseudo-segments, or a call without a state, sets its own tables) and the clause's queries, boost and filter ids.
// The caller adds the tiles, the output and k / cap
slg::VsScanParams vs_scan_base(const VsCall &vc, const VsArgs &a, uint32_t c) {
  slg::VsScanParams sp{};
  if (vc.S) {
    const IndexState &S = *vc.S;
    sp.segs = S.d_segs.as<slg::SegDev>();
    sp.reject_table = S.d_reject_table.as<const uint32_t *>();
    sp.doc_base = S.d_doc_base.as<uint32_t>();
    sp.n_segs = (uint32_t)S.segs.size();
    sp.n_filters = (uint32_t)S.filters.size();
  }
  sp.vsegs = vc.vsegs[c];
  sp.dim = vc.dim[c];
  sp.nq = vc.nq;
  sp.qvecs = a.qvecs;
  sp.q_stride = vc.q_floats;
  sp.q_off = vc.coff[c];
  sp.qvec4 = vs_qvec4(vc, a, c);
  sp.boost = a.boost;
  sp.n_clauses = vc.n_clauses;
  sp.clause = c;
  sp.q_filter = a.q_filter;
  return sp;
}

// the one place that names the scan kernels' instantiations.  The parameter type picks the kernel: VsScanParams the
// f32 scan, VsScanBf16Params the bf16 first pass, VsIvfScanParams the scan of the IVF work table (top-k form only)
template <int METRIC, bool TOPK, typename P>
void vs_launch_scan_as(const P &p, dim3 grid, size_t lds, hipStream_t st) {
  if constexpr (std::is_same<P, slg::VsScanParams>::value)
    launch_kernel_lds(slg::vs_scan_kernel<METRIC, TOPK>, p, grid, 256, lds, st);
  else if constexpr (std::is_same<P, slg::VsScanBf16Params>::value)
    launch_kernel_lds(slg::vs_scan_bf16_kernel<METRIC, TOPK>, p, grid, 256, lds, st);
  else if constexpr (TOPK)
    launch_kernel_lds(slg::vs_ivf_scan_kernel<METRIC, true>, p, grid, 256, lds, st);
  else
    throw SlgError(SLG_ERR_UNSUPPORTED, "the store form of the IVF scan is not built");
}
template <typename P>
void vs_launch_scan(int32_t metric, bool topk, const P &p, dim3 grid, size_t lds, hipStream_t st) {
  if (metric == 0)
    topk ? vs_launch_scan_as<0, true>(p, grid, lds, st) : vs_launch_scan_as<0, false>(p, grid, lds, st);
  else
    topk ? vs_launch_scan_as<1, true>(p, grid, lds, st) : vs_launch_scan_as<1, false>(p, grid, lds, st);
}

// a segment's list object with its tables allocated: the centroid table (not yet filled), the list ids 0, 1, ..
std::shared_ptr<VecListSeg> vs_new_lists(slg_index *ix, uint32_t n_lists, uint32_t dim) {
  auto ls = std::make_shared<VecListSeg>();
  ls->n_lists = n_lists;
  ls->dim = dim;
  ls->list_begin.alloc(((size_t)n_lists + 1) * 4, &ix->pool);
  ls->centroids.alloc((size_t)n_lists * dim * 4, &ix->pool);
  ls->iota.alloc((size_t)n_lists * 4, &ix->pool);
  std::vector<uint32_t> iota(n_lists);
  for (uint32_t i = 0; i < n_lists; i++) iota[i] = i;
  SLG_HIP(hipMemcpy(ls->iota.p, iota.data(), (size_t)n_lists * 4, hipMemcpyHostToDevice));
  return ls;
}

// ---- the list of every row: an exact scan with the rows as queries, the centroids as the docs of one
//      pseudo-segment without tombstones, and a top-1 ----
// (the tables point at ls's centroid table: run() assigns to whatever it holds at that point of the stream)
struct IvfAssign {
  DevBuf d_cseg, d_pseg, d_cbase, partials;
  slg::VsScanParams sp{};
  const float *d_values = nullptr;
  uint32_t n_rows = 0, n_chunks = 0;
  int32_t metric = 0;
  size_t lds = 0;
  static constexpr uint32_t batch = 65536;  // rows of one scan

  IvfAssign(slg_index *ix, const VecListSeg &ls, const float *values, uint32_t rows, int32_t metric_)
      : d_values(values), n_rows(rows), metric(metric_) {
    const uint32_t n_lists = ls.n_lists, dim = ls.dim;
    const slg::VecSegDev cseg{ls.iota.as<uint32_t>(), ls.centroids.as<float>(), n_lists, dim, metric, 0u};
    const slg::SegDev pseg{};
    const uint32_t cbase[2] = {0u, n_lists};
    d_cseg.alloc(sizeof(cseg), &ix->pool);
    d_pseg.alloc(sizeof(pseg), &ix->pool);
    d_cbase.alloc(sizeof(cbase), &ix->pool);
    SLG_HIP(hipMemcpy(d_cseg.p, &cseg, sizeof(cseg), hipMemcpyHostToDevice));
    SLG_HIP(hipMemcpy(d_pseg.p, &pseg, sizeof(pseg), hipMemcpyHostToDevice));
    SLG_HIP(hipMemcpy(d_cbase.p, cbase, sizeof(cbase), hipMemcpyHostToDevice));
    const uint32_t n_tiles = (n_lists + slg::kVsTileDocs - 1) / slg::kVsTileDocs;
    lds = slg::vs_scan_lds_bytes(true, slg::kVsBufCapNarrow);
    if (!n_rows) return;
    const uint32_t b_rows = std::min(batch, n_rows), qtiles = (b_rows + slg::kVsTileQ - 1) / slg::kVsTileQ;
    const VsChunks ch = vs_round_chunks(vs_resident_groups(ix, lds), qtiles, n_tiles, n_tiles);
    n_chunks = ch.n_chunks;
    partials.alloc((size_t)b_rows * n_chunks * slg::kVsSmallK * 8, &ix->pool);
    // the rows are the query vectors of a one-clause call without an index state: the tables are the pseudo-segment's
    VsCall vc;
    vc.n_clauses = 1;
    vc.dim[0] = vc.q_floats = dim;
    vc.vsegs[0] = d_cseg.as<slg::VecSegDev>();
    VsArgs a{};
    a.qvecs = d_values;
    sp = vs_scan_base(vc, a, 0);
    sp.segs = d_pseg.as<slg::SegDev>();
    sp.doc_base = d_cbase.as<uint32_t>();
    sp.n_segs = 1;
    sp.tile_end = n_tiles;
    sp.tiles_per_block = ch.tpb;
    sp.n_chunks = n_chunks;
    sp.out = partials.as<uint64_t>();
    sp.k = 1;
    sp.cap = slg::kVsBufCapNarrow;
  }

  void run(uint32_t *row_list, hipStream_t st) {
    for (uint32_t r0 = 0; r0 < n_rows; r0 += batch) {
      const uint32_t nr = std::min(batch, n_rows - r0);
      sp.nq = nr;
      sp.qvecs = d_values + (size_t)r0 * sp.dim;
      vs_launch_scan(metric, true, sp, dim3((nr + slg::kVsTileQ - 1) / slg::kVsTileQ, n_chunks), lds, st);
      slg::IvfBestParams bp{partials.as<uint64_t>(), nr, n_chunks, row_list + r0};
      hipLaunchKernelGGL(slg::vs_ivf_best_kernel, dim3((nr + 255) / 256), dim3(256), 0, st, bp);
      SLG_HIP(hipGetLastError());
    }
  }
};

// ---- the lists of an assignment: count per (list, doc range), prefix per list, exclusive scan of the lengths,
//      ordered fill.  lb: list_begin as read back ----
void vs_build_lists(slg_index *ix, const uint32_t *d_offsets, uint32_t n_docs, const uint32_t *row_list,
                    VecListSeg *ls, std::vector<uint32_t> *lb_out) {
  const hipStream_t st = ix->stream;
  const uint32_t n_lists = ls->n_lists;
  DevBuf doc_list, table, lens;
  const uint32_t max_ranges = std::max<uint32_t>(std::min<uint32_t>(slg::kIvfMaxRanges, (16u << 20) / n_lists), 1u);
  uint32_t range_docs = std::max<uint32_t>(slg::kIvfRangeDocs, (n_docs + max_ranges - 1) / max_ranges);
  range_docs = (range_docs + 63u) / 64u * 64u;
  const uint32_t n_ranges = std::max<uint32_t>((n_docs + range_docs - 1) / range_docs, 1u);
  doc_list.alloc(std::max<size_t>(n_docs, 1) * 4, &ix->pool);
  table.alloc((size_t)n_lists * n_ranges * 4, &ix->pool);
  lens.alloc((size_t)n_lists * 4, &ix->pool);
  SLG_HIP(hipMemsetAsync(table.p, 0, (size_t)n_lists * n_ranges * 4, st));
  slg::IvfBuildParams bp{};
  bp.offsets = d_offsets;
  bp.row_list = row_list;
  bp.doc_list = doc_list.as<uint32_t>();
  bp.table = table.as<uint32_t>();
  bp.lens = lens.as<uint32_t>();
  bp.list_begin = ls->list_begin.as<uint32_t>();
  bp.n_docs = n_docs;
  bp.n_lists = n_lists;
  bp.n_ranges = n_ranges;
  bp.range_docs = range_docs;
  if (n_docs) hipLaunchKernelGGL(slg::vs_ivf_count_kernel, dim3((n_docs + 255) / 256), dim3(256), 0, st, bp);
  hipLaunchKernelGGL(slg::vs_ivf_prefix_kernel, dim3((n_lists + 255) / 256), dim3(256), 0, st, bp);
  slg::IvfScanParams xp{lens.as<uint32_t>(), ls->list_begin.as<uint32_t>(), n_lists};
  hipLaunchKernelGGL(slg::vs_ivf_exscan_kernel, dim3(1), dim3(slg::kIvfScanThreads), 0, st, xp);
  SLG_HIP(hipGetLastError());
  std::vector<uint32_t> &lb = *lb_out;
  lb.assign((size_t)n_lists + 1, 0u);
  SLG_HIP(hipMemcpyAsync(lb.data(), ls->list_begin.p, lb.size() * 4, hipMemcpyDeviceToHost, st));
  SLG_HIP(hipStreamSynchronize(st));
  ls->n_listed = lb[n_lists];
  SLG_REQUIRE(ls->n_listed <= n_docs, "the lists hold more docs than the segment");
  ls->max_len = 0;
  for (uint32_t l = 0; l < n_lists; l++) ls->max_len = std::max(ls->max_len, lb[l + 1] - lb[l]);
  const size_t docs_bytes = std::max<size_t>(ls->n_listed, 1) * 4;
  if (ls->docs.bytes != docs_bytes) ls->docs.alloc(docs_bytes, &ix->pool);
  bp.docs = ls->docs.as<uint32_t>();
  if (n_docs) hipLaunchKernelGGL(slg::vs_ivf_fill_kernel, dim3(n_ranges), dim3(64), 0, st, bp);
  SLG_HIP(hipGetLastError());
  SLG_HIP(hipStreamSynchronize(st));
}

}  // namespace

std::shared_ptr<VecListSeg> slghost::vs_cluster_store(slg_index *ix, const uint32_t *d_offsets, const float *d_values,
                                                      uint32_t n_docs, uint32_t n_rows, uint32_t dim, int32_t metric,
                                                      const float *centroids, uint32_t n_lists) {
  auto ls = vs_new_lists(ix, n_lists, dim);
  SLG_HIP(hipMemcpy(ls->centroids.p, centroids, (size_t)n_lists * dim * 4, hipMemcpyHostToDevice));
  DevBuf row_list;
  row_list.alloc(std::max<size_t>(n_rows, 1) * 4, &ix->pool);
  IvfAssign assign(ix, *ls, d_values, n_rows, metric);
  assign.run(row_list.as<uint32_t>(), ix->stream);
  std::vector<uint32_t> lb;
  vs_build_lists(ix, d_offsets, n_docs, row_list.as<uint32_t>(), ls.get(), &lb);
  return ls;
}

std::shared_ptr<VecListSeg> slghost::vs_train_store(slg_index *ix, const uint32_t *d_offsets, const float *d_values,
                                                    uint32_t n_docs, uint32_t n_rows, uint32_t dim, int32_t metric,
                                                    const float *init, uint32_t n_lists, uint32_t iters,
                                                    slg_vector_train_stats *stats) {
  const hipStream_t st = ix->stream;
  auto ls = vs_new_lists(ix, n_lists, dim);
  const size_t c_bytes = (size_t)n_lists * dim * 4;
  if (init) {
    SLG_HIP(hipMemcpy(ls->centroids.p, init, c_bytes, hipMemcpyHostToDevice));
  } else {
    slg::IvfStartParams sp{d_values, ls->centroids.as<float>(), n_rows, n_lists, dim};
    const uint64_t n = (uint64_t)n_lists * dim;
    hipLaunchKernelGGL(slg::vs_ivf_start_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, sp);
    SLG_HIP(hipGetLastError());
  }
  // the scratch of the loop: all of it is released when the call returns
  DevBuf rl[2], d_moved, next, d_items, d_item_begin, partial;
  rl[0].alloc(std::max<size_t>(n_rows, 1) * 4, &ix->pool);
  rl[1].alloc(std::max<size_t>(n_rows, 1) * 4, &ix->pool);
  d_moved.alloc(4, &ix->pool);
  next.alloc(c_bytes, &ix->pool);
  d_item_begin.alloc(((size_t)n_lists + 1) * 4, &ix->pool);
  IvfAssign assign(ix, *ls, d_values, n_rows, metric);
  std::vector<uint32_t> lb, item_begin((size_t)n_lists + 1);
  std::vector<slg::IvfSumItem> items;
  uint32_t cur = 0, iters_run = 0, moved_last = 0;
  bool stopped = false;
  for (uint32_t t = 1; t <= iters; t++) {
    assign.run(rl[cur].as<uint32_t>(), st);
    uint32_t moved = n_rows;
    if (t > 1) {
      SLG_HIP(hipMemsetAsync(d_moved.p, 0, 4, st));
      slg::IvfMovedParams mp{rl[cur].as<uint32_t>(), rl[cur ^ 1].as<uint32_t>(), n_rows, d_moved.as<uint32_t>()};
      if (n_rows) hipLaunchKernelGGL(slg::vs_ivf_moved_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, st, mp);
      SLG_HIP(hipGetLastError());
      SLG_HIP(hipMemcpyAsync(&moved, d_moved.p, 4, hipMemcpyDeviceToHost, st));
      SLG_HIP(hipStreamSynchronize(st));
    }
    moved_last = moved;
    if (t > 1 && moved == 0) {  // a fixed point: the lists of the previous step are those of these centroids
      stopped = true;
      break;
    }
    vs_build_lists(ix, d_offsets, n_docs, rl[cur].as<uint32_t>(), ls.get(), &lb);
    // the work table: one item per (list, chunk of its docs)
    items.clear();
    for (uint32_t l = 0; l < n_lists; l++) {
      item_begin[l] = (uint32_t)items.size();
      for (uint32_t d = lb[l]; d < lb[l + 1]; d += slg::kIvfTrainChunk)
        items.push_back(slg::IvfSumItem{d, std::min(d + slg::kIvfTrainChunk, lb[l + 1])});
    }
    const uint32_t n_items = (uint32_t)items.size();
    item_begin[n_lists] = n_items;
    SLG_HIP(hipMemcpy(d_item_begin.p, item_begin.data(), item_begin.size() * 4, hipMemcpyHostToDevice));
    if (n_items) {
      if (d_items.bytes < (size_t)n_items * sizeof(slg::IvfSumItem))
        d_items.alloc((size_t)n_items * sizeof(slg::IvfSumItem) * 5 / 4, &ix->pool);
      if (partial.bytes < (size_t)n_items * dim * 8) partial.alloc((size_t)n_items * dim * 8 * 5 / 4, &ix->pool);
      SLG_HIP(hipMemcpy(d_items.p, items.data(), (size_t)n_items * sizeof(slg::IvfSumItem), hipMemcpyHostToDevice));
      slg::IvfSumParams sp{d_items.as<slg::IvfSumItem>(), ls->docs.as<uint32_t>(), d_offsets, d_values,
                           partial.as<double>(), n_items, n_docs, n_rows, dim};
      hipLaunchKernelGGL(slg::vs_ivf_sum_kernel, dim3(std::min<uint32_t>(n_items, 1u << 20)),
                         dim3(slg::kIvfTrainThreads), 0, st, sp);
    }
    slg::IvfCentroidParams cp{partial.as<double>(), d_item_begin.as<uint32_t>(), ls->list_begin.as<uint32_t>(),
                              ls->centroids.as<float>(), next.as<float>(), n_lists, dim, metric};
    hipLaunchKernelGGL(slg::vs_ivf_centroid_kernel, dim3(n_lists), dim3(slg::kIvfTrainThreads), 0, st, cp);
    SLG_HIP(hipGetLastError());
    SLG_HIP(hipMemcpyAsync(ls->centroids.p, next.p, c_bytes, hipMemcpyDeviceToDevice, st));
    iters_run++;
    cur ^= 1;
  }
  if (!stopped) {  // the lists of the final centroids
    assign.run(rl[cur].as<uint32_t>(), st);
    vs_build_lists(ix, d_offsets, n_docs, rl[cur].as<uint32_t>(), ls.get(), &lb);
  }
  SLG_HIP(hipStreamSynchronize(st));
  if (stats) {
    stats->iters_run = iters_run;
    stats->moved = iters ? moved_last : 0u;
    stats->empty_lists = 0;
    for (uint32_t l = 0; l < n_lists; l++) stats->empty_lists += lb[l + 1] == lb[l] ? 1u : 0u;
    stats->max_len = ls->max_len;
  }
  return ls;
}

namespace {

// one block of scratch as a list of arrays.  A layout takes its arrays from a Carver in order: over no block it only
// counts, over the block it binds the pointers, so a block's size and its pointers come from one list.  Every array
// starts 8-byte aligned; bytes() adds a slack of 256
struct Carver {
  unsigned char *base;  // null: count only
  size_t off = 0;
  explicit Carver(void *block) : base(static_cast<unsigned char *>(block)) {}
  template <typename T>
  T *take(size_t n) {
    T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
    off += (n * sizeof(T) + 7) / 8 * 8;
    return p;
  }
  size_t bytes() const { return off + 256; }
};
// the index's vs_scratch, grown by a quarter beyond what a call needs
void *vs_scratch(slg_index *ix, size_t bytes) {
  if (ix->vs_scratch.bytes < bytes) ix->vs_scratch.alloc(bytes + bytes / 4, &ix->pool);
  return ix->vs_scratch.p;
}

// how the scans of one call cut the flat doc space for lists of K keys: K <= kVsSmallK = the fused top-k epilogue
// over n_chunks doc chunks of one round of resident workgroups, else chunks of chunk_docs docs + select
struct VsPlan {
  bool small = false, bf16 = false;
  uint32_t n_tiles = 0, qtiles = 0, n_chunks = 0, tpb = 0, chunk_docs = 0, cap = 0;
  size_t n_in = 0;  // keys of the scans' output, all clauses
  size_t lds(bool topk) const { return bf16 ? slg::va_scan_lds_bytes(topk, cap) : slg::vs_scan_lds_bytes(topk, cap); }
};

VsPlan vs_plan(slg_index *ix, const VsCall &vc, uint32_t K, bool bf16) {
  const IndexState &S = *vc.S;
  VsPlan pl;
  pl.bf16 = bf16;
  const uint32_t n_tiles = (uint32_t)((S.total_docs + slg::kVsTileDocs - 1) / slg::kVsTileDocs);
  pl.n_tiles = n_tiles;
  pl.qtiles = (vc.nq + slg::kVsTileQ - 1) / slg::kVsTileQ;
  pl.small = K <= slg::kVsSmallK;
  pl.cap = K <= slg::kVsSmallK / 2 ? slg::kVsBufCapNarrow : slg::kVsBufCap;
  if (pl.small && pl.n_tiles) {
    // (by_vgprs 2 for vs_scan_bf16_kernel, whose 197 registers leave two waves per SIMD); the partial lists of a
    // query sort in LDS with its running list
    const VsChunks ch =
        vs_round_chunks(vs_resident_groups(ix, pl.lds(true), bf16 ? 2u : 3u), pl.qtiles, n_tiles,
                        std::min<uint32_t>(n_tiles, (slg::kVsSortCap - slg::kVsSmallK) / slg::kVsSmallK));
    pl.n_chunks = ch.n_chunks;
    pl.tpb = ch.tpb;
  } else if (!pl.small) {
    pl.chunk_docs = ((slg::kVsSortCap - K) / slg::kVsTileDocs) * slg::kVsTileDocs;
  }
  pl.n_in = pl.small ? (size_t)vc.n_clauses * vc.nq * pl.n_chunks * slg::kVsSmallK : (size_t)vc.nq * pl.chunk_docs;
  return pl;
}

// one launch of vs_select_kernel over (nq, n_cl) lists: sel without its pass (n_in keys per query, final_)
void vs_select_pass(slg::VsSelectParams sel, uint32_t n_in, uint32_t sort_n, bool final_, dim3 grid, hipStream_t st) {
  sel.n_in = n_in;
  sel.final_ = final_ ? 1u : 0u;
  launch_kernel_lds(slg::vs_select_kernel, sel, grid, slg::kVsSortThreads, (size_t)slg::vs_pow2(sel.k + sort_n) * 8, st);
}
slg::VsSelectParams vs_select_params(uint64_t *run, uint32_t *run_cnt, uint64_t *dlist, const uint64_t *in, uint32_t nq,
                                     uint32_t K, uint32_t c0, uint32_t stride) {
  slg::VsSelectParams sel{};
  sel.run = run;
  sel.run_cnt = run_cnt;
  sel.dlist = dlist;
  sel.nq = nq;
  sel.k = K;
  sel.in = in;
  sel.c0 = c0;
  sel.in_stride = stride;
  return sel;
}
void vs_select(uint64_t *run, uint32_t *run_cnt, uint64_t *dlist, const uint64_t *in, uint32_t nq, uint32_t K,
               uint32_t c0, uint32_t n_cl, uint32_t n_in_q, uint32_t stride, bool final_, hipStream_t st) {
  vs_select_pass(vs_select_params(run, run_cnt, dlist, in, nq, K, c0, stride), n_in_q, n_in_q, final_, dim3(nq, n_cl),
                 st);
}
// `total` keys per query fold into the running lists in passes of kVsSortCap - k keys, which sort in LDS with the
// running list; the last pass is final.  sel.in_off (the hybrid call's keys): the kernel cuts every query's pass from
// its own count, and every pass has the LDS of the first
void vs_fold(slg::VsSelectParams sel, uint64_t total, dim3 grid, hipStream_t st) {
  const uint32_t fold_n = slg::kVsSortCap - sel.k;
  const uint64_t passes = std::max<uint64_t>((total + fold_n - 1) / fold_n, 1);
  const uint64_t *in = sel.in;
  for (uint64_t t = 0; t < passes; t++) {
    const uint64_t o = t * fold_n;
    const bool final_ = t + 1 == passes;
    if (sel.in_off) {
      sel.in_skip = (uint32_t)o;
      vs_select_pass(sel, fold_n, (uint32_t)std::min<uint64_t>(total, fold_n), final_, grid, st);
    } else {
      const uint32_t n = (uint32_t)std::min<uint64_t>(fold_n, total - o);
      sel.in = in + o;
      vs_select_pass(sel, n, n, final_, grid, st);
    }
  }
}

// the clause lists of one call on st: per (clause, query) the best K keys in run (best first, run_cnt of them;
// zeroed by the caller) and, final_, sorted by doc in dlist.  The exact scan, or (pl.bf16) the scan of the bf16 copies
void vs_lists(const VsCall &vc, const VsArgs &a, const VsPlan &pl, uint32_t K, uint64_t *run, uint32_t *run_cnt,
              uint64_t *dlist, uint64_t *in, bool final_, hipStream_t st) {
  const uint32_t nq = vc.nq, NC = vc.n_clauses;
  slg::VsScanBf16Params bp[SLG_MAX_VECTOR_CLAUSES];
  for (uint32_t c = 0; c < NC; c++) {
    bp[c].s = vs_scan_base(vc, a, c);
    bp[c].s.k = K;
    bp[c].s.cap = pl.cap;
    bp[c].csegs = vc.csegs[c];
  }
  auto scan = [&](uint32_t c, bool topk, dim3 grid) {
    if (pl.bf16)
      vs_launch_scan(vc.metric[c], topk, bp[c], grid, pl.lds(topk), st);
    else
      vs_launch_scan(vc.metric[c], topk, bp[c].s, grid, pl.lds(topk), st);
  };
  if (pl.small) {
    for (uint32_t c = 0; c < NC && pl.n_chunks; c++) {
      slg::VsScanParams &sp = bp[c].s;
      sp.tile_begin = 0;
      sp.tile_end = pl.n_tiles;
      sp.tiles_per_block = pl.tpb;
      sp.n_chunks = pl.n_chunks;
      sp.out = in + (size_t)c * nq * pl.n_chunks * slg::kVsSmallK;
      scan(c, true, dim3(pl.qtiles, pl.n_chunks));
    }
    vs_select(run, run_cnt, dlist, in, nq, K, 0, NC, pl.n_chunks * slg::kVsSmallK, pl.n_chunks * slg::kVsSmallK,
              final_, st);
  } else {
    const uint32_t tiles_per_chunk = pl.chunk_docs / slg::kVsTileDocs;
    const uint32_t steps = std::max<uint32_t>((pl.n_tiles + tiles_per_chunk - 1) / tiles_per_chunk, 1u);
    for (uint32_t s = 0; s < steps; s++) {
      const uint32_t t0 = s * tiles_per_chunk, t1 = std::min<uint32_t>(t0 + tiles_per_chunk, pl.n_tiles);
      for (uint32_t c = 0; c < NC; c++) {
        slg::VsScanParams &sp = bp[c].s;
        sp.out = in;
        sp.out_stride = pl.chunk_docs;
        sp.tiles_per_block = 1;
        sp.tile_begin = t0;
        sp.tile_end = t1;
        if (t1 > t0) scan(c, false, dim3(pl.qtiles, t1 - t0));
        vs_select(run, run_cnt, dlist, in, nq, K, c, 1, (t1 > t0 ? t1 - t0 : 0) * slg::kVsTileDocs, pl.chunk_docs,
                  final_ && s + 1 == steps, st);
      }
    }
  }
}

// the fields vs_blend_kernel reads in both of its forms: the clause lists (K keys each, sorted by doc), the sort
// space of the union (P keys a query; ukeys when they do not fit LDS) and the outputs
slg::VsBlendParams vs_blend_params(const VsCall &vc, const VsArgs &a, const uint64_t *dlist, const uint32_t *run_cnt,
                                   uint32_t K, uint64_t *ukeys, uint32_t P) {
  const IndexState &S = *vc.S;
  slg::VsBlendParams bp{};
  bp.dlist = dlist;
  bp.run_cnt = run_cnt;
  bp.nq = vc.nq;
  bp.k = K;
  bp.n_clauses = vc.n_clauses;
  bp.alpha = a.alpha;
  for (uint32_t c = 0; c < vc.n_clauses; c++) bp.metric[c] = vc.metric[c];
  bp.doc_base = S.d_doc_base.as<uint32_t>();
  bp.n_segs = (uint32_t)S.segs.size();
  bp.ukeys = ukeys;
  bp.P = P;
  bp.k_out = vc.k_out;
  bp.out_doc = a.out_doc;
  bp.out_seg = a.out_seg;
  bp.out_score = a.out_score;
  bp.out_vec = a.out_vec;
  bp.out_count = a.out_count;
  bp.out_total = a.out_total;
  return bp;
}
// union of the clause lists, blend, top k_out
void vs_blend(const VsCall &vc, const VsArgs &a, const uint64_t *dlist, const uint32_t *run_cnt, uint32_t K,
              uint64_t *ukeys, uint32_t P, hipStream_t st) {
  launch_kernel_lds(slg::vs_blend_kernel<false>, vs_blend_params(vc, a, dlist, run_cnt, K, ukeys, P), dim3(vc.nq),
                    slg::kVsSortThreads, P > slg::kVsSortCap ? 0 : (size_t)P * 8, st);
}

// (slg_vector_search_batch_ivf*) what one clause's steps need of vs_scratch, from what the host knows: nq, the
// probes of a query, the field's lists, its longest list and its unclustered segments
struct IvfPlan {
  uint32_t nq = 0;
  uint32_t P = 0;            // probes of a query: min(nprobe, lists of the field)
  uint32_t list_chunks = 0, list_chunk_docs = 0, slots_q = 0, n_ext = 0, items_cap = 0;
  uint32_t coarse_docs = 0;  // lists of one coarse scan + select step
  size_t n_probe_keys = 0, n_coarse = 0, n_partial = 0;
  size_t bytes() const;      // of its work area (IvfWork)
};
IvfPlan ivf_plan(const VsCall &vc, uint32_t c, uint32_t nprobe) {
  const VecListField &vl = *vc.lists[c];
  IvfPlan pl;
  pl.nq = vc.nq;
  pl.P = std::min(nprobe, vl.total_lists);
  pl.list_chunks = std::max<uint32_t>(std::min<uint32_t>(slg::kIvfListChunks, (vl.max_len + 1023u) / 1024u), 1u);
  pl.list_chunk_docs = std::max<uint32_t>(((vl.max_len + pl.list_chunks - 1) / pl.list_chunks + slg::kVsTileDocs - 1) /
                                              slg::kVsTileDocs * slg::kVsTileDocs, slg::kVsTileDocs);
  pl.slots_q = pl.P * pl.list_chunks + vl.uncl_slots;
  pl.n_ext = vl.total_lists + vl.n_uncl;
  const uint32_t qtiles = (vc.nq + slg::kVsTileQ - 1) / slg::kVsTileQ;
  // a list's items: its query tiles x its chunks; all lists: at most the probes / 64 + one tile per probed list
  const uint64_t pairs = (uint64_t)vc.nq * pl.P;
  const uint64_t items = (pairs / slg::kVsTileQ + std::min<uint64_t>(vl.total_lists, pairs)) * pl.list_chunks +
                         (uint64_t)qtiles * vl.uncl_slots;
  SLG_REQUIRE(pairs < 0x7FFFFFFFull && items < 0x7FFFFFFFull, "too many (query, probed list) pairs in one call");
  pl.items_cap = (uint32_t)items;
  pl.coarse_docs = std::min<uint32_t>(((slg::kVsSortCap - pl.P) / slg::kVsTileDocs) * slg::kVsTileDocs,
                                      (vl.total_lists + slg::kVsTileDocs - 1) / slg::kVsTileDocs * slg::kVsTileDocs);
  pl.n_probe_keys = pairs;
  pl.n_coarse = (size_t)vc.nq * pl.coarse_docs;
  pl.n_partial = (size_t)vc.nq * pl.slots_q * slg::kVsSmallK;
  return pl;
}
// the work area of one clause's steps
struct IvfWork {
  uint64_t *probes, *coarse, *partials;
  slg::IvfItem *items;
  uint2 *pairs;
  uint32_t *cnt;  // [n_ext] the lists' query counts, then [n_ext] the fill cursors: zeroed together
  uint32_t *goff, *ioff, *n_items;
  uint32_t *probe_cnt;  // [nq] the coarse select's counts
  size_t lay(const IvfPlan &pl, void *block) {
    Carver c(block);
    probes = c.take<uint64_t>(pl.n_probe_keys);
    coarse = c.take<uint64_t>(pl.n_coarse);
    partials = c.take<uint64_t>(pl.n_partial);
    items = c.take<slg::IvfItem>(pl.items_cap);
    pairs = c.take<uint2>(pl.n_probe_keys);
    cnt = c.take<uint32_t>(2 * (size_t)pl.n_ext);
    goff = c.take<uint32_t>((size_t)pl.n_ext + 1);
    ioff = c.take<uint32_t>((size_t)pl.n_ext + 1);
    n_items = c.take<uint32_t>(1);
    probe_cnt = c.take<uint32_t>(pl.nq);
    return c.off;
  }
};
size_t IvfPlan::bytes() const { return IvfWork().lay(*this, nullptr); }

// the clause lists of one IVF call on st (run / run_cnt zeroed by the caller; work: the clause-by-clause work area)
void vs_lists_ivf(slg_index *ix, const VsCall &vc, const VsArgs &a, uint32_t nprobe, uint64_t *run, uint32_t *run_cnt,
                  uint64_t *dlist, void *work, hipStream_t st) {
  const IndexState &S = *vc.S;
  const uint32_t nq = vc.nq, NC = vc.n_clauses, K = vc.cand;
  const uint32_t cap = K <= slg::kVsSmallK / 2 ? slg::kVsBufCapNarrow : slg::kVsBufCap;
  const size_t scan_lds = slg::vs_ivf_scan_lds_bytes(cap);
  const uint32_t qtiles = (nq + slg::kVsTileQ - 1) / slg::kVsTileQ;
  for (uint32_t c = 0; c < NC; c++) {
    const VecListField &vl = *vc.lists[c];
    const IvfPlan pl = ivf_plan(vc, c, nprobe);
    IvfWork w;
    w.lay(pl, work);
    // every counter of the steps, and the partial slots no item writes
    SLG_HIP(hipMemsetAsync(w.cnt, 0, (2 * (size_t)pl.n_ext) * 4, st));
    SLG_HIP(hipMemsetAsync(w.n_items, 0, 4, st));
    SLG_HIP(hipMemsetAsync(w.partials, 0, pl.n_partial * 8, st));
    SLG_HIP(hipMemsetAsync(w.probes, 0, pl.n_probe_keys * 8, st));
    // ---- coarse step: the exact scan's store form over the centroid tables (pseudo-segments without tombstones
    //      or filters), the best P lists of each query ----
    slg::VsScanParams sp = vs_scan_base(vc, a, c);
    sp.vsegs = vl.d_csegs.as<slg::VecSegDev>();
    sp.segs = vl.d_psegs.as<slg::SegDev>();
    sp.doc_base = vl.d_list_base.as<uint32_t>();
    sp.reject_table = nullptr;
    sp.n_filters = 0;
    sp.q_filter = nullptr;
    sp.tiles_per_block = 1;
    sp.out = w.coarse;
    sp.out_stride = pl.coarse_docs;
    const uint32_t n_tiles = (vl.total_lists + slg::kVsTileDocs - 1) / slg::kVsTileDocs;
    const uint32_t step_tiles = pl.coarse_docs / slg::kVsTileDocs;
    SLG_HIP(hipMemsetAsync(w.probe_cnt, 0, (size_t)nq * 4, st));
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += step_tiles) {
      const uint32_t t1 = std::min(t0 + step_tiles, n_tiles);
      sp.tile_begin = t0;
      sp.tile_end = t1;
      vs_launch_scan(vc.metric[c], false, sp, dim3(qtiles, t1 - t0), slg::vs_scan_lds_bytes(false, 0), st);
      vs_select(w.probes, w.probe_cnt, nullptr, w.coarse, nq, pl.P, 0, 1, (t1 - t0) * slg::kVsTileDocs, pl.coarse_docs,
                false, st);
    }
    // ---- inversion: the probes as per-list query groups, and the work table ----
    const slg::IvfPlanParams ip{w.probes, vl.d_lsegs.as<slg::VecListDev>(), vl.d_list_base.as<uint32_t>(),
                                vl.d_uncl.as<slg::IvfUncl>(), (uint32_t)S.segs.size(), vl.total_lists, vl.n_uncl, nq,
                                pl.P, pl.list_chunk_docs, pl.list_chunks, w.cnt, w.cnt + pl.n_ext, w.goff, w.ioff,
                                w.n_items, w.pairs, w.items, pl.items_cap};
    const uint32_t n_pairs = nq * pl.P;
    hipLaunchKernelGGL(slg::vs_ivf_probe_count_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, st, ip);
    hipLaunchKernelGGL(slg::vs_ivf_plan_kernel, dim3(1), dim3(slg::kIvfScanThreads), 0, st, ip);
    hipLaunchKernelGGL(slg::vs_ivf_items_kernel, dim3((std::max(n_pairs, pl.n_ext) + 255) / 256), dim3(256), 0, st, ip);
    SLG_HIP(hipGetLastError());
    // ---- the scan of the work table by one round of resident workgroups ----
    slg::VsIvfScanParams xp{};
    xp.s = vs_scan_base(vc, a, c);
    xp.s.out = w.partials;
    xp.s.k = K;
    xp.s.cap = cap;
    xp.lsegs = ip.lsegs;
    xp.items = w.items;
    xp.n_items = w.n_items;
    xp.pairs = w.pairs;
    xp.slots_q = pl.slots_q;
    // (profiles/vsearch_ivf_resource_usage.txt: the cosine form's registers leave two waves per SIMD, the L2 form's one)
    const uint32_t groups = vs_resident_groups(ix, scan_lds, vc.metric[c] == 0 ? 2u : 1u);
    vs_launch_scan(vc.metric[c], true, xp, dim3(std::min<uint32_t>(groups, std::max<uint32_t>(pl.items_cap, 1u))),
                   scan_lds, st);
    // ---- a query's partials fold into its clause list ----
    const uint32_t n_in = pl.slots_q * slg::kVsSmallK;
    const size_t qc0 = (size_t)c * nq;
    vs_fold(vs_select_params(run + qc0 * K, run_cnt + qc0, dlist + qc0 * K, w.partials, nq, K, 0, n_in), n_in,
            dim3(nq, 1), st);
  }
}

// the kernels of one IVF call on st: per clause the coarse step, the scan of the probed lists and the fold; blend
void vs_run_ivf(slg_index *ix, const VsCall &vc, const VsArgs &a, uint32_t nprobe, hipStream_t st) {
  const uint32_t nq = vc.nq, NC = vc.n_clauses, K = vc.cand;
  const size_t n_run = (size_t)NC * nq * K, n_cnt = (size_t)NC * nq;
  const uint32_t P = slg::vs_pow2(NC * K);  // (K <= kVsSmallK: the union sorts in LDS)
  size_t work = 0;
  for (uint32_t c = 0; c < NC; c++) work = std::max(work, ivf_plan(vc, c, nprobe).bytes());
  uint64_t *run = nullptr, *dlist = nullptr;
  unsigned char *wk = nullptr;
  uint32_t *run_cnt = nullptr;
  auto lay = [&](void *block) {
    Carver c(block);
    run = c.take<uint64_t>(n_run);
    dlist = c.take<uint64_t>(n_run);
    wk = c.take<unsigned char>(work);
    run_cnt = c.take<uint32_t>(n_cnt);
    return c.bytes();
  };
  lay(vs_scratch(ix, lay(nullptr)));
  SLG_HIP(hipMemsetAsync(run_cnt, 0, n_cnt * 4, st));
  vs_lists_ivf(ix, vc, a, nprobe, run, run_cnt, dlist, wk, st);
  vs_blend(vc, a, dlist, run_cnt, K, nullptr, P, st);
}

// the kernels of one scan call on st.  refine 0: the exact search; else the two-pass one: lists of `refine` keys from
// the bf16 copies, their exact scores, the best cand_size
void vs_run_scan(slg_index *ix, const VsCall &vc, const VsArgs &a, uint32_t refine, hipStream_t st) {
  const uint32_t nq = vc.nq, NC = vc.n_clauses, K = vc.cand, R = refine ? refine : K;
  const VsPlan pl = vs_plan(ix, vc, R, refine != 0);
  const size_t n_run = (size_t)NC * nq * K, n_first = refine ? (size_t)NC * nq * R : 0, n_cnt = (size_t)NC * nq;
  const uint32_t P = slg::vs_pow2(NC * K);
  uint64_t *run = nullptr, *dlist = nullptr, *first = nullptr, *in = nullptr, *ukeys = nullptr;
  uint32_t *run_cnt = nullptr;  // [n_cnt], then the first pass's counts: zeroed together
  auto lay = [&](void *block) {
    Carver c(block);
    run = c.take<uint64_t>(n_run);
    dlist = c.take<uint64_t>(n_run);
    first = c.take<uint64_t>(n_first);
    in = c.take<uint64_t>(std::max<size_t>(pl.n_in, 1));
    ukeys = c.take<uint64_t>(P > slg::kVsSortCap ? (size_t)nq * P : 0);
    run_cnt = c.take<uint32_t>(2 * n_cnt);
    return c.bytes();
  };
  lay(vs_scratch(ix, lay(nullptr)));
  uint32_t *first_cnt = run_cnt + n_cnt;
  SLG_HIP(hipMemsetAsync(run_cnt, 0, 2 * n_cnt * 4, st));
  if (!refine) {
    vs_lists(vc, a, pl, K, run, run_cnt, dlist, in, true, st);
  } else {
    vs_lists(vc, a, pl, R, first, first_cnt, nullptr, in, false, st);
    const IndexState &S = *vc.S;
    slg::VsRefineParams rp{};
    rp.doc_base = S.d_doc_base.as<uint32_t>();
    rp.n_segs = (uint32_t)S.segs.size();
    rp.nq = nq;
    rp.qvecs = a.qvecs;
    rp.q_stride = vc.q_floats;
    rp.boost = a.boost;
    rp.n_clauses = NC;
    rp.run = first;
    rp.run_cnt = first_cnt;
    rp.k = R;
    for (uint32_t c = 0; c < NC; c++) {
      rp.vsegs = vc.vsegs[c];
      rp.dim = vc.dim[c];
      rp.q_off = vc.coff[c];
      rp.qvec4 = vs_qvec4(vc, a, c);
      rp.clause = c;
      if (vc.metric[c] == 0)
        hipLaunchKernelGGL(slg::vs_refine_kernel<0>, dim3(nq), dim3(256), 0, st, rp);
      else
        hipLaunchKernelGGL(slg::vs_refine_kernel<1>, dim3(nq), dim3(256), 0, st, rp);
      SLG_HIP(hipGetLastError());
    }
    // the refined keys fold into the final lists
    vs_fold(vs_select_params(run, run_cnt, dlist, first, nq, K, 0, R), R, dim3(nq, NC), st);
  }
  vs_blend(vc, a, dlist, run_cnt, K, ukeys, P, st);
}

// the kernels of one call on st, device arrays in a (the caller holds ix->mu and the device).  nprobe != 0: the search
// over the fields' inverted-file lists; else the scans of the flat space, exact (refine 0) or two-pass
void vs_run(slg_index *ix, const VsCall &vc, const VsArgs &a, uint32_t refine, uint32_t nprobe, hipStream_t st) {
  if (nprobe)
    vs_run_ivf(ix, vc, a, nprobe, st);
  else
    vs_run_scan(ix, vc, a, refine, st);
}

// (slg_vector_search_batch_approx*) a bf16 copy of every clause's field; refine against cand_size
void vs_prepare_approx(uint32_t n_clauses, const uint32_t *clause_field, VsCall *vc) {
  const IndexState &S = *vc->S;
  for (uint32_t c = 0; c < n_clauses; c++) {
    const auto it = S.vcopies.find(clause_field[c]);
    SLG_REQUIRE(it != S.vcopies.end(), "vector field " + std::to_string(clause_field[c]) +
                                           " has no bf16 copy (slg_index_quantize_vector_field)");
    vc->csegs[c] = it->second->d_csegs.as<slg::VecCopyDev>();
  }
}
// (slg_vector_search_batch_ivf*) nprobe and cand_size, checked first; then the lists of every clause's field
void vs_check_ivf(uint32_t cand_size, uint32_t nprobe) {
  if (nprobe < 1 || nprobe > SLG_MAX_VECTOR_PROBES)
    throw SlgError(SLG_ERR_UNSUPPORTED, "nprobe outside 1..SLG_MAX_VECTOR_PROBES");
  if (cand_size > slg::kVsSmallK)
    throw SlgError(SLG_ERR_UNSUPPORTED, "cand_size > 64 is not built for the IVF search: use slg_vector_search_batch "
                                        "or slg_vector_search_batch_approx");
}
void vs_prepare_ivf(uint32_t n_clauses, const uint32_t *clause_field, VsCall *vc) {
  const IndexState &S = *vc->S;
  for (uint32_t c = 0; c < n_clauses; c++) {
    const auto it = S.vlists.find(clause_field[c]);
    SLG_REQUIRE(it != S.vlists.end() && it->second->total_lists != 0,
                "vector field " + std::to_string(clause_field[c]) + " has no lists (slg_index_cluster_vector_field)");
    vc->lists[c] = it->second.get();
  }
}
void vs_check_refine(uint32_t cand_size, uint32_t refine) {
  if (refine < cand_size || refine > SLG_MAX_VECTOR_CANDIDATES)
    throw SlgError(SLG_ERR_UNSUPPORTED, "refine outside cand_size..SLG_MAX_VECTOR_CANDIDATES");
}

// which of the three searches an entry point runs; `extra` is its own integer: none, refine, nprobe
enum class VsKind { Exact, Approx, Ivf };

// one entry point of the family.  device: the arrays of a are device memory and the call is asynchronous on the index
// stream; else host arrays: checks, pooled device buffers, H2D, the kernels, D2H and a wait, all on the index stream
// (Staging: slg_host.hpp)
int vs_entry(VsKind kind, bool device, slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
             uint32_t cand_size, uint32_t extra, uint32_t k_out, const VsArgs &a) {
  return guarded([&] {
    if (kind == VsKind::Approx) vs_check_refine(cand_size, extra);
    if (kind == VsKind::Ivf) vs_check_ivf(cand_size, extra);
    const uint32_t refine = kind == VsKind::Approx ? extra : 0u, nprobe = kind == VsKind::Ivf ? extra : 0u;
    VsCall vc;
    if (!vs_prepare(ix, nq, n_clauses, clause_field, cand_size, k_out, a, !device, &vc)) return;
    if (refine) vs_prepare_approx(n_clauses, clause_field, &vc);
    if (nprobe) vs_prepare_ivf(n_clauses, clause_field, &vc);
    const hipStream_t st = ix->stream;
    if (device) {
      std::lock_guard<std::mutex> lk(ix->mu);
      DeviceGuard g(ix->device);
      vs_run(ix, vc, a, refine, nprobe, st);
      return;
    }
    DeviceGuard g(ix->device);
    const size_t nqc = (size_t)nq * n_clauses, no = (size_t)nq * k_out;
    Staging sg(&ix->pool, st);
    VsArgs d{};
    d.qvecs = sg.up(a.qvecs, (size_t)nq * vc.q_floats);
    d.alpha = sg.up(a.alpha, nqc);
    if (a.boost) d.boost = sg.up(a.boost, nqc);
    if (a.q_filter) d.q_filter = sg.up(a.q_filter, nq);
    d.out_doc = sg.up<uint32_t>(nullptr, no);
    d.out_seg = sg.up<uint32_t>(nullptr, no);
    d.out_score = sg.up<float>(nullptr, no);
    d.out_vec = sg.up<float>(nullptr, no);
    d.out_count = sg.up<uint32_t>(nullptr, nq);
    d.out_total = sg.up<uint64_t>(nullptr, nq);
    {
      std::lock_guard<std::mutex> lk(ix->mu);
      vs_run(ix, vc, d, refine, nprobe, st);
    }
    sg.down(a.out_doc, d.out_doc, no);
    sg.down(a.out_seg, d.out_seg, no);
    sg.down(a.out_score, d.out_score, no);
    sg.down(a.out_vec, d.out_vec, no);
    sg.down(a.out_count, d.out_count, nq);
    sg.down(a.out_total, d.out_total, nq);
    SLG_HIP(hipStreamSynchronize(st));
  });
}
}  // namespace

size_t slghost::hy_work_layout(const VsCall &vc, uint32_t bm_k, void *base, HyWork *w) {
  const size_t n_run = (size_t)vc.n_clauses * vc.nq * vc.cand, n_cnt = (size_t)vc.n_clauses * vc.nq;
  const uint32_t P = slg::vs_pow2(vc.n_clauses * vc.cand + bm_k), Pb = slg::vs_pow2(std::max<uint32_t>(bm_k, 1u));
  HyWork lw{};
  Carver c(w ? base : nullptr);
  lw.run = c.take<uint64_t>(n_run);
  lw.dlist = c.take<uint64_t>(n_run);
  // the union keys sort in LDS while they fit, and the BM25 hits behind them while both do
  lw.ukeys = c.take<uint64_t>(P > slg::kVsSortCap ? (size_t)vc.nq * P : 0);
  lw.bkeys = c.take<uint64_t>(P + Pb > slg::kVsSortCap ? (size_t)vc.nq * Pb : 0);
  lw.cnt = c.take<uint32_t>(2 * n_cnt);  // (hy_fold reads the key counts right behind the run counts)
  lw.P = P;
  lw.Pb = Pb;
  if (w) *w = lw;
  return c.bytes();
}

void slghost::hy_fold(const VsCall &vc, const HyWork &w, const HyKeys &k, hipStream_t st) {
  slg::VsSelectParams sel = vs_select_params(w.run, w.cnt, w.dlist, k.keys, vc.nq, vc.cand, 0, (uint32_t)k.stride);
  sel.in_off = k.q_cand;
  sel.in_cnt = w.cnt + (size_t)vc.n_clauses * vc.nq;
  sel.in_base = k.slot_lo;
  sel.q0 = k.q_lo;
  vs_fold(sel, k.max_cap, dim3(k.q_hi - k.q_lo, vc.n_clauses), st);
}

void slghost::hy_blend(const VsCall &vc, const VsArgs &a, const HyWork &w, const uint32_t *bm_doc,
                       const uint32_t *bm_seg, const float *bm_score, const uint32_t *bm_count, uint32_t bm_k,
                       hipStream_t st) {
  slg::VsBlendParams bp = vs_blend_params(vc, a, w.dlist, w.cnt, vc.cand, w.ukeys, w.P);
  bp.bm_doc = bm_doc;
  bp.bm_seg = bm_seg;
  bp.bm_score = bm_score;
  bp.bm_count = bm_count;
  bp.bkeys = w.bkeys;
  bp.bm_k = bm_k;
  bp.Pb = w.Pb;
  bp.bm_lds = w.P + w.Pb <= slg::kVsSortCap ? 1u : 0u;
  const size_t lds = ((w.P > slg::kVsSortCap ? 0 : (size_t)w.P) + (bp.bm_lds ? w.Pb : 0)) * 8;
  launch_kernel_lds(slg::vs_blend_kernel<true>, bp, dim3(vc.nq), slg::kVsSortThreads, lds, st);
}

extern "C" {

int slg_vector_search_batch(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                            const float *qvecs, const float *alpha, const float *boost, const int32_t *q_filter,
                            uint32_t cand_size, uint32_t k_out, uint32_t *out_doc, uint32_t *out_seg,
                            float *out_score, float *out_vec_score, uint32_t *out_count, uint64_t *out_total) {
  return vs_entry(VsKind::Exact, false, ix, nq, n_clauses, clause_field, cand_size, 0, k_out,
                  {qvecs, alpha, boost, q_filter, out_doc, out_seg, out_score, out_vec_score, out_count, out_total});
}

int slg_vector_search_batch_device(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                                   const float *d_qvecs, const float *d_alpha, const float *d_boost,
                                   const int32_t *d_q_filter, uint32_t cand_size, uint32_t k_out,
                                   uint32_t *d_out_doc, uint32_t *d_out_seg, float *d_out_score,
                                   float *d_out_vec_score, uint32_t *d_out_count, uint64_t *d_out_total) {
  return vs_entry(VsKind::Exact, true, ix, nq, n_clauses, clause_field, cand_size, 0, k_out,
                  {d_qvecs, d_alpha, d_boost, d_q_filter, d_out_doc, d_out_seg, d_out_score, d_out_vec_score,
                   d_out_count, d_out_total});
}

int slg_vector_search_batch_approx(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                                   const float *qvecs, const float *alpha, const float *boost, const int32_t *q_filter,
                                   uint32_t cand_size, uint32_t refine, uint32_t k_out, uint32_t *out_doc,
                                   uint32_t *out_seg, float *out_score, float *out_vec_score, uint32_t *out_count,
                                   uint64_t *out_total) {
  return vs_entry(VsKind::Approx, false, ix, nq, n_clauses, clause_field, cand_size, refine, k_out,
                  {qvecs, alpha, boost, q_filter, out_doc, out_seg, out_score, out_vec_score, out_count, out_total});
}

int slg_vector_search_batch_approx_device(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                                          const float *d_qvecs, const float *d_alpha, const float *d_boost,
                                          const int32_t *d_q_filter, uint32_t cand_size, uint32_t refine,
                                          uint32_t k_out, uint32_t *d_out_doc, uint32_t *d_out_seg,
                                          float *d_out_score, float *d_out_vec_score, uint32_t *d_out_count,
                                          uint64_t *d_out_total) {
  return vs_entry(VsKind::Approx, true, ix, nq, n_clauses, clause_field, cand_size, refine, k_out,
                  {d_qvecs, d_alpha, d_boost, d_q_filter, d_out_doc, d_out_seg, d_out_score, d_out_vec_score,
                   d_out_count, d_out_total});
}

int slg_vector_search_batch_ivf(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                                const float *qvecs, const float *alpha, const float *boost, const int32_t *q_filter,
                                uint32_t cand_size, uint32_t nprobe, uint32_t k_out, uint32_t *out_doc,
                                uint32_t *out_seg, float *out_score, float *out_vec_score, uint32_t *out_count,
                                uint64_t *out_total) {
  return vs_entry(VsKind::Ivf, false, ix, nq, n_clauses, clause_field, cand_size, nprobe, k_out,
                  {qvecs, alpha, boost, q_filter, out_doc, out_seg, out_score, out_vec_score, out_count, out_total});
}

int slg_vector_search_batch_ivf_device(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                                       const float *d_qvecs, const float *d_alpha, const float *d_boost,
                                       const int32_t *d_q_filter, uint32_t cand_size, uint32_t nprobe, uint32_t k_out,
                                       uint32_t *d_out_doc, uint32_t *d_out_seg, float *d_out_score,
                                       float *d_out_vec_score, uint32_t *d_out_count, uint64_t *d_out_total) {
  return vs_entry(VsKind::Ivf, true, ix, nq, n_clauses, clause_field, cand_size, nprobe, k_out,
                  {d_qvecs, d_alpha, d_boost, d_q_filter, d_out_doc, d_out_seg, d_out_score, d_out_vec_score,
                   d_out_count, d_out_total});
}

}  // extern "C"
