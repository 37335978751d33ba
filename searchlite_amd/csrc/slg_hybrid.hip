// slg_hybrid.hip — hybrid text + vector search (slg_batch_prepare_hybrid, slg_batch_hybrid_device,
// slg_search_batch_hybrid; the gather kernel: slg_hybrid.hpp; fold and blend: slg_vsearch.hip).
#include "slg_host.hpp"

#include "slg_hybrid.hpp"

using namespace slghost;

namespace {

// Bytes of gathered keys (8 B x candidate slots x clauses) a call holds at a time: the key area comes from the
// index's buffer pool, so it takes at most a quarter of the pool's cap (slg_tuning.pool_cap_mb) and at most
// 1 GiB; the queries of a batch are processed in ranges that fit.
uint64_t key_budget_bytes(const slg_index *ix) {
  return std::max<uint64_t>(std::min<uint64_t>(ix->pool.cap / 4, 1ull << 30), 1ull << 20);
}

// One hybrid call on a batch: every check, against the state the batch was prepared on.  false: nothing to do
bool hy_check(slg_batch *b, uint32_t n_clauses, const uint32_t *clause_field, uint32_t cand_size, uint32_t k_out,
              const VsArgs &a, VsCall *vc) {
  SLG_REQUIRE_LIVE(b);
  SLG_REQUIRE(b->hybrid, "not a hybrid batch (slg_batch_prepare_hybrid)");
  if (!vs_prepare(b->idx, b->nq, n_clauses, clause_field, cand_size, k_out, a, false, vc, b->snap)) return false;
  SLG_REQUIRE(b->launched, "the batch has not run (slg_batch_run)");
  uint32_t lds_floats = 0;
  for (uint32_t c = 0; c < n_clauses; c++) lds_floats += (vc->dim[c] + 3u) & ~3u;
  if (lds_floats > slg::kHyLdsFloats)
    throw SlgError(SLG_ERR_UNSUPPORTED, "the clause vectors of a query exceed the gather kernel's LDS budget");
  return true;
}

// the ranges of queries whose keys fit the budget: [first, last) pairs; a query that does not fit alone: OOM
std::vector<std::pair<uint32_t, uint32_t>> key_ranges(const slg_batch *b, uint32_t n_clauses, uint64_t budget) {
  std::vector<std::pair<uint32_t, uint32_t>> out;
  const uint64_t max_slots = std::min<uint64_t>(budget / (8ull * n_clauses), 0xFFFFFFFFull);
  uint32_t q0 = 0;
  while (q0 < b->nq) {
    uint32_t q1 = q0;
    while (q1 < b->nq && b->q_cand[q1 + 1] - b->q_cand[q0] <= max_slots) q1++;
    if (q1 == q0)
      throw SlgError(SLG_ERR_OOM, "query " + std::to_string(q0) + ": the keys of its matched docs (" +
                                      std::to_string((b->q_cand[q0 + 1] - b->q_cand[q0]) * 8 * n_clauses) +
                                      " bytes) exceed the key work area");
    out.emplace_back(q0, q1);
    q0 = q1;
  }
  return out;
}

// the kernels of one call on the batch's stream, device arrays in a (the caller holds ix->mu and the device)
void hy_run(slg_batch *b, const VsCall &vc, const VsArgs &a, hipStream_t st) {
  slg_index *ix = b->idx;
  const IndexState &S = *vc.S;
  const uint32_t nq = vc.nq, NC = vc.n_clauses;
  // ---- everything that can fail for want of memory, before the first launch ----
  const auto ranges = key_ranges(b, NC, key_budget_bytes(ix));
  uint64_t max_slots = 0;
  for (const auto &r : ranges) max_slots = std::max(max_slots, b->q_cand[r.second] - b->q_cand[r.first]);
  const size_t key_bytes = (size_t)std::max<uint64_t>(max_slots, 1) * NC * 8;
  const size_t work_bytes = hy_work_layout(vc, b->k, nullptr, nullptr);
  // (a block that grows goes back to the pool: an earlier call's kernels on this stream may still use it)
  if ((b->d_hy_keys.p && b->d_hy_keys.bytes < key_bytes) || (b->d_hy_work.p && b->d_hy_work.bytes < work_bytes))
    SLG_HIP(hipStreamSynchronize(st));
  if (b->d_hy_keys.bytes < key_bytes) b->d_hy_keys.alloc_pooled(&ix->pool, key_bytes);
  if (b->d_hy_work.bytes < work_bytes) b->d_hy_work.alloc_pooled(&ix->pool, work_bytes);
  HyWork w{};
  hy_work_layout(vc, b->k, b->d_hy_work.p, &w);
  uint32_t *key_cnt = w.cnt + (size_t)NC * nq;
  SLG_HIP(hipMemsetAsync(w.cnt, 0, 2 * (size_t)NC * nq * 4, st));

  slg::HyGatherParams gp{};
  gp.cand = b->d_cand.as<uint2>();
  gp.slice_cbeg = b->d_slice_cbeg.as<uint64_t>();
  gp.slice_ccnt = b->d_slice_ccnt.as<uint32_t>();
  gp.slice_seg = b->d_slice_seg;
  gp.slice_sq = b->d_slice_sq;
  gp.sq = b->d_sq;
  gp.n_slices = b->n_slices;
  gp.n_segs = (uint32_t)S.segs.size();
  gp.segs = S.d_segs.as<slg::SegDev>();
  gp.q_filter = b->d_q_filter.as<uint32_t>();
  gp.reject_table = S.d_reject_table.as<const uint32_t *>();
  gp.doc_base = S.d_doc_base.as<uint32_t>();
  gp.qvecs = a.qvecs;
  gp.boost = a.boost;
  gp.q_stride = vc.q_floats;
  gp.n_clauses = NC;
  gp.nq = nq;
  uint32_t lds_floats = 0;
  for (uint32_t c = 0; c < NC; c++) {
    gp.cl[c] = slg::HyClause{vc.vsegs[c], vc.dim[c], lds_floats, vc.coff[c], vc.metric[c]};
    lds_floats += (vc.dim[c] + 3u) & ~3u;
  }
  gp.q_cand = b->d_q_cand.as<uint64_t>();
  gp.keys = b->d_hy_keys.as<uint64_t>();
  gp.key_cnt = key_cnt;
  for (const auto &r : ranges) {
    gp.slot_lo = b->q_cand[r.first];
    gp.slot_hi = b->q_cand[r.second];
    const uint64_t slots = gp.slot_hi - gp.slot_lo;
    uint64_t max_cap = 0;
    for (uint32_t q = r.first; q < r.second; q++) max_cap = std::max(max_cap, b->q_cand[q + 1] - b->q_cand[q]);
    if (slots && b->n_slices) {
      // enough workgroups to fill the device also when few docs match: shorter spans, down to one wave's
      uint32_t span = slg::kHySpanMax;
      while (span > 64 && slots / span < 2048) span >>= 1;
      gp.span = span;
      launch_kernel_lds(slg::hy_gather_kernel, gp, dim3((uint32_t)((slots + span - 1) / span)),
                        std::min<uint32_t>(span, slg::kHyThreads), (size_t)std::max<uint32_t>(lds_floats, 4) * 4, st);
    }
    hy_fold(vc, w, HyKeys{gp.keys, slots, gp.slot_lo, max_cap, gp.q_cand, r.first, r.second}, st);
  }
  hy_blend(vc, a, w, b->d_out_doc, b->d_out_seg, b->d_out_score, b->d_out_count, b->k, st);
}

}  // namespace

extern "C" {

slg_batch *slg_batch_prepare_hybrid(slg_index *ix, uint32_t nq, const uint32_t *q_offsets,
                                    const uint32_t *q_term_ids, const float *q_weights,
                                    const slg_score_plans *plans, const int32_t *q_filter, uint32_t k,
                                    int strategy) {
  PrepareRequest r{ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy};
  r.hybrid = true;
  return prepare_impl(r);
}

int slg_batch_hybrid_device(slg_batch *b, uint32_t n_clauses, const uint32_t *clause_field, const float *d_qvecs,
                            const float *d_alpha, const float *d_boost, uint32_t cand_size, uint32_t k_out,
                            uint32_t *d_out_doc, uint32_t *d_out_seg, float *d_out_score, float *d_out_vec_score,
                            uint32_t *d_out_count, uint64_t *d_out_total) {
  return guarded([&] {
    const VsArgs a{d_qvecs, d_alpha, d_boost, nullptr,        d_out_doc,
                   d_out_seg, d_out_score, d_out_vec_score, d_out_count, d_out_total};
    VsCall vc;
    if (!hy_check(b, n_clauses, clause_field, cand_size, k_out, a, &vc)) return;
    std::lock_guard<std::mutex> lk(b->idx->mu);
    DeviceGuard g(b->idx->device);
    hy_run(b, vc, a, batch_stream(b));
  });
}

int slg_search_batch_hybrid(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                            const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                            uint32_t k, int strategy, uint32_t n_clauses, const uint32_t *clause_field,
                            const float *qvecs, const float *alpha, const float *boost, uint32_t cand_size,
                            uint32_t k_out, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                            float *out_vec_score, uint32_t *out_count, uint64_t *out_total) {
  const VsArgs h{qvecs, alpha, boost, nullptr, out_doc, out_seg, out_score, out_vec_score, out_count, out_total};
  // the vector side's checks come first: nothing is planned or staged for a call they refuse
  int rc = guarded([&] {
    VsCall vc;
    (void)vs_prepare(ix, nq, n_clauses, clause_field, cand_size, k_out, h, false, &vc);
  });
  if (rc != SLG_OK) return rc;
  slg_batch *b = slg_batch_prepare_hybrid(ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy);
  if (!b) return last_error().code;
  rc = slg_batch_run(b);
  if (rc == SLG_OK)
    rc = guarded([&] {
      VsCall vc;
      if (!hy_check(b, n_clauses, clause_field, cand_size, k_out, h, &vc)) return;
      const size_t nqc = (size_t)nq * n_clauses, no = (size_t)nq * k_out;
      DeviceGuard g(ix->device);
      const hipStream_t st = locked_stream(b);
      Staging sg(&ix->pool, st);
      VsArgs d{};
      d.qvecs = sg.up(h.qvecs, (size_t)nq * vc.q_floats);
      d.alpha = sg.up(h.alpha, nqc);
      if (h.boost) d.boost = sg.up(h.boost, nqc);
      d.out_doc = sg.up<uint32_t>(nullptr, no);
      d.out_seg = sg.up<uint32_t>(nullptr, no);
      d.out_score = sg.up<float>(nullptr, no);
      d.out_vec = sg.up<float>(nullptr, no);
      d.out_count = sg.up<uint32_t>(nullptr, nq);
      d.out_total = sg.up<uint64_t>(nullptr, nq);
      {
        std::lock_guard<std::mutex> lk(ix->mu);
        hy_run(b, vc, d, st);
      }
      sg.down(h.out_doc, d.out_doc, no);
      sg.down(h.out_seg, d.out_seg, no);
      sg.down(h.out_score, d.out_score, no);
      sg.down(h.out_vec, d.out_vec, no);
      sg.down(h.out_count, d.out_count, nq);
      sg.down(h.out_total, d.out_total, nq);
      uint32_t flag = 0;  // the index's error word as the batch's last kernel saw it (as slg_batch_fetch)
      SLG_HIP(hipMemcpyAsync(&flag, ResultBlock(nq, k).flag(b->d_out.as<uint32_t>()), 4, hipMemcpyDeviceToHost, st));
      SLG_HIP(hipStreamSynchronize(st));
      if (flag != 0u)
        throw SlgError(SLG_ERR_INTERNAL, "a scoring wave gave up on a round (chunk-loop guard): results are incomplete");
    });
  KeepLastError keep;
  slg_batch_destroy(b);
  return rc;
}

}  // extern "C"
