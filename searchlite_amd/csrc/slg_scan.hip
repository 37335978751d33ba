// slg_scan.hip — scan batches (slg_batch_prepare_scan): match_all, constant_score and rank_feature at the root.
// The planned slice tables onto the device, the launch of scan_kernel in the place of a batch's partition and
// scoring kernels, and the one-call form.  (The checks of a spec and the tables themselves: slg_plan.cpp,
// check_scan / plan_scan.)  Everything behind the candidates — the selects, the matched counts, the aggregation
// kernels, fetch — is what slg_batch_run and the fetch calls do for every batch.
#include "slg_host.hpp"

#include "slg_scan.hpp"

using namespace slghost;

void slghost::scan_launch(slg_batch *b, hipStream_t st) {
  // (every run counts anew: the kernel adds each slice's docs to its query's two counters)
  SLG_HIP(hipMemsetAsync(b->d_q_scored.p, 0, (size_t)b->nq * 4, st));
  SLG_HIP(hipMemsetAsync(b->d_matched.p, 0, (size_t)b->nq * 8, st));
  if (b->n_slices == 0) {
    // no segment has a doc: no kernel of this batch writes a row in score order (slg_batch_run zeroes the counts;
    // the sorted select and the aggregation kernels run over the empty slice ranges as they do for any batch)
    if (!b->sorted && b->k > 0)
      SLG_HIP(hipMemsetAsync(b->d_out.p, 0, ResultBlock(b->nq, b->k).words_with_flag() * 4, st));
    return;
  }
  if (!b->cand_mode) throw SlgError(SLG_ERR_INTERNAL, "a scan batch was not planned in candidates mode");
  slg::ScanParams p{};
  unsigned char *base = b->d_desc.as<unsigned char>();
  p.segs = b->snap->d_segs.as<slg::SegDev>();
  p.slices = reinterpret_cast<const slg::ScanSlice *>(base);
  base += (size_t)b->n_slices * sizeof(slg::ScanSlice);
  p.queries = reinterpret_cast<const slg::ScanQuery *>(base);
  base += (size_t)b->nq * sizeof(slg::ScanQuery);
  p.cols = reinterpret_cast<const slg::ColumnDev *>(base);
  p.q_filter = b->d_q_filter.as<uint32_t>();
  p.reject_table = b->snap->d_reject_table.as<const uint32_t *>();
  p.cand = b->d_cand.as<uint2>();
  p.slice_cbeg = b->d_slice_cbeg.as<uint64_t>();
  p.slice_ccnt = b->d_slice_ccnt.as<uint32_t>();
  p.q_scored = b->d_q_scored.as<uint32_t>();
  p.q_matched = b->d_matched.as<unsigned long long>();
  p.n_slices = b->n_slices;
  p.n_segs = (uint32_t)b->snap->segs.size();
  constexpr uint32_t per_block = slg::kScanThreads / 64;
  const dim3 grid((b->n_slices + per_block - 1) / per_block), block(slg::kScanThreads);
  if (b->scan_full) hipLaunchKernelGGL(slg::scan_kernel<true>, grid, block, 0, st, p);
  else hipLaunchKernelGGL(slg::scan_kernel<false>, grid, block, 0, st, p);
  SLG_HIP(hipGetLastError());
}

extern "C" {

slg_batch *slg_batch_prepare_scan(slg_index *ix, uint32_t nq, const slg_scan_spec *spec, const int32_t *q_filter,
                                  const slg_sort_spec *sort, const slg_agg_spec *aggs, uint32_t k) {
  return prepare_guarded([&](slg_batch *&b) {
    slgplan::check_scan(spec, nq, k);  // (what needs no index comes first, as every argument check)
    if (aggs) agg_check_spec(aggs);
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    check_sort_spec(sort);
    const std::shared_ptr<const IndexState> snap = ix->snapshot();
    const std::vector<char> filter_live = filter_liveness(*snap);
    std::vector<uint32_t> seg_docs(snap->segs.size());
    for (size_t s = 0; s < snap->segs.size(); s++) seg_docs[s] = snap->segs[s]->n_docs;
    SortBinding sorting;
    if (sort) sorting = bind_sort(*snap, *sort, "", "part ");
    slgplan::ScanPlan plan;
    slgplan::plan_scan(seg_docs, fscore_field_views(*snap), filter_live.data(), filter_live.size(), nq, *spec, q_filter,
                       sort != nullptr || aggs != nullptr, k, plan);

    DeviceGuard g(ix->device);
    b = new slg_batch();
    b->idx = ix;
    b->snap = snap;
    b->nq = nq;
    b->k = k;
    b->score_k = k;
    b->strategy = SLG_STRATEGY_BM25;
    b->q_postings.assign(nq, 0);
    b->scan = true;
    b->scan_full = plan.full;
    b->cand_mode = true;
    b->n_slices = (uint32_t)plan.slices.size();
    // the tables of the scan, then what the selects read of any batch (all naturally aligned in this order)
    upload_image(b->d_desc, &ix->pool,
                 {image_part(plan.slices), image_part(plan.queries), image_part(plan.cols), image_part(plan.qrefs),
                  image_part(plan.slice_seg)});
    {
      const unsigned char *db = b->d_desc.as<unsigned char>() + plan.slices.size() * sizeof(slg::ScanSlice) +
                                plan.queries.size() * sizeof(slg::ScanQuery) + plan.cols.size() * sizeof(slg::ColumnDev);
      b->d_queries = reinterpret_cast<const slg::QueryRef *>(db);
      b->d_slice_seg = reinterpret_cast<const uint32_t *>(db + plan.qrefs.size() * sizeof(slg::QueryRef));
    }
    b->d_cand.alloc_pooled(&ix->pool, (size_t)(plan.cand_total + 1) * 8);
    b->d_slice_cbeg.alloc_pooled(&ix->pool, (size_t)b->n_slices * 8);
    if (b->n_slices)
      SLG_HIP(hipMemcpy(b->d_slice_cbeg.p, plan.slice_cbeg.data(), (size_t)b->n_slices * 8, hipMemcpyHostToDevice));
    b->d_slice_ccnt.alloc_pooled(&ix->pool, (size_t)b->n_slices * 4);
    b->d_q_scored.alloc_pooled(&ix->pool, (size_t)nq * 4);
    attach_select_buffers(b, plan.q_filter, sort, sorting, true);  // (scan_kernel counts every query's matched docs)
    if (aggs) agg_attach(b, *aggs);
  });
}

int slg_batch_scan_info(const slg_batch *b, uint32_t *out_variant, uint32_t *out_slices, uint32_t *out_slice_docs) {
  return guarded([&] {
    SLG_REQUIRE(b != nullptr, "batch is NULL");
    SLG_REQUIRE(b->scan, "not a scan batch (slg_batch_prepare_scan)");
    if (out_variant) *out_variant = b->n_slices == 0 ? 0u : (b->scan_full ? 2u : 1u);
    if (out_slices) *out_slices = b->n_slices;
    if (out_slice_docs) *out_slice_docs = slg::kScanSliceDocs;
  });
}

int slg_search_batch_scan(slg_index *ix, uint32_t nq, const slg_scan_spec *spec, const int32_t *q_filter,
                          const slg_sort_spec *sort, const slg_agg_spec *aggs, uint32_t k, uint32_t *out_doc,
                          uint32_t *out_seg, float *out_score, uint32_t *out_count, uint64_t *out_matched,
                          uint64_t *counts, slg_agg_stats *stats, uint64_t *values) {
  HostOut o{out_doc, out_seg, out_score, out_count, nullptr, out_matched, nullptr, counts, stats};
  o.agg_values = values;
  return run_to_host(slg_batch_prepare_scan(ix, nq, spec, q_filter, sort, aggs, k), o);
}

}  // extern "C"
