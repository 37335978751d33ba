// slg_vsearch.hip — exact vector-only search (slg_vector_search_batch*; kernels: slg_vsearch.hpp).
#include "slg_host.hpp"

#include "slg_vsearch.hpp"

using namespace slghost;

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

namespace {

// the kernels of one call on st, device arrays in a (the caller holds ix->mu and the device)
void vs_run(slg_index *ix, const VsCall &vc, const VsArgs &a, hipStream_t st) {
  const IndexState &S = *vc.S;
  const uint32_t nq = vc.nq, NC = vc.n_clauses, K = vc.cand;
  const uint32_t n_segs = (uint32_t)S.segs.size();
  const uint64_t n_tiles64 = (S.total_docs + slg::kVsTileDocs - 1) / slg::kVsTileDocs;
  const uint32_t n_tiles = (uint32_t)n_tiles64;
  const uint32_t qtiles = (nq + slg::kVsTileQ - 1) / slg::kVsTileQ;
  const bool small = K <= slg::kVsSmallK;
  // the path is chosen from cand_size: small = fused top-k epilogue, else chunks of docs + select
  uint32_t n_chunks = 0, tpb = 0, chunk_docs = 0;
  const uint32_t cap = K <= slg::kVsSmallK / 2 ? slg::kVsBufCapNarrow : slg::kVsBufCap;
  if (small && n_tiles) {
    // one round of resident workgroups: as many as the LDS of a CU holds (at most 3, the VGPR bound)
    int n_cu = 0;
    SLG_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ix->device));
    const uint32_t per_cu = std::min<uint32_t>(3u, (uint32_t)((160u << 10) / slg::vs_scan_lds_bytes(true, cap)));
    const uint32_t target = std::max<uint32_t>((uint32_t)n_cu, 1u) * std::max<uint32_t>(per_cu, 1u);
    n_chunks = std::min<uint32_t>(std::max<uint32_t>((target + qtiles - 1) / qtiles, 1u),
                                  std::min<uint32_t>(n_tiles, (slg::kVsSortCap - slg::kVsSmallK) / slg::kVsSmallK));
    tpb = (n_tiles + n_chunks - 1) / n_chunks;
    n_chunks = (n_tiles + tpb - 1) / tpb;
  } else if (!small) {
    chunk_docs = ((slg::kVsSortCap - K) / slg::kVsTileDocs) * slg::kVsTileDocs;
  }
  const size_t n_run = (size_t)NC * nq * K;
  const size_t n_in = small ? (size_t)NC * nq * n_chunks * slg::kVsSmallK : (size_t)nq * chunk_docs;
  const uint32_t P = slg::vs_pow2(NC * K);
  const size_t n_u = P > slg::kVsSortCap ? (size_t)nq * P : 0;
  const size_t bytes = (2 * n_run + std::max<size_t>(n_in, 1) + n_u) * 8 + (size_t)NC * nq * 4 + 256;
  if (ix->vs_scratch.bytes < bytes) ix->vs_scratch.alloc(bytes + bytes / 4, &ix->pool);
  uint64_t *run = ix->vs_scratch.as<uint64_t>(), *dlist = run + n_run, *in = dlist + n_run;
  uint64_t *ukeys = in + std::max<size_t>(n_in, 1);
  uint32_t *run_cnt = reinterpret_cast<uint32_t *>(ukeys + n_u);
  SLG_HIP(hipMemsetAsync(run_cnt, 0, (size_t)NC * nq * 4, st));

  slg::VsScanParams sp{};
  sp.segs = S.d_segs.as<slg::SegDev>();
  sp.reject_table = S.d_reject_table.as<const uint32_t *>();
  sp.doc_base = S.d_doc_base.as<uint32_t>();
  sp.n_segs = n_segs;
  sp.n_filters = (uint32_t)S.filters.size();
  sp.nq = nq;
  sp.qvecs = a.qvecs;
  sp.q_stride = vc.q_floats;
  sp.boost = a.boost;
  sp.n_clauses = NC;
  sp.q_filter = a.q_filter;
  sp.k = K;
  sp.cap = cap;
  auto scan = [&](uint32_t c, bool topk, dim3 grid) {
    sp.vsegs = vc.vsegs[c];
    sp.dim = vc.dim[c];
    sp.q_off = vc.coff[c];
    sp.clause = c;
    sp.qvec4 = (vc.q_floats % 4 == 0 && vc.coff[c] % 4 == 0 && ((uintptr_t)a.qvecs & 15) == 0) ? 1u : 0u;
    const size_t lds = slg::vs_scan_lds_bytes(topk, sp.cap);
    if (vc.metric[c] == 0)
      topk ? launch_kernel_lds(slg::vs_scan_kernel<0, true>, sp, grid, 256, lds, st)
           : launch_kernel_lds(slg::vs_scan_kernel<0, false>, sp, grid, 256, lds, st);
    else
      topk ? launch_kernel_lds(slg::vs_scan_kernel<1, true>, sp, grid, 256, lds, st)
           : launch_kernel_lds(slg::vs_scan_kernel<1, false>, sp, grid, 256, lds, st);
  };
  slg::VsSelectParams sel{};
  sel.run = run;
  sel.run_cnt = run_cnt;
  sel.dlist = dlist;
  sel.nq = nq;
  sel.k = K;
  sel.in = in;
  auto select = [&](uint32_t c0, uint32_t n_cl, uint32_t n_in_q, uint32_t stride, bool final_) {
    sel.c0 = c0;
    sel.n_in = n_in_q;
    sel.in_stride = stride;
    sel.final_ = final_ ? 1u : 0u;
    const size_t lds = (size_t)slg::vs_pow2(K + n_in_q) * 8;
    launch_kernel_lds(slg::vs_select_kernel, sel, dim3(nq, n_cl), slg::kVsSortThreads, lds, st);
  };
  if (small) {
    sp.tile_begin = 0;
    sp.tile_end = n_tiles;
    sp.tiles_per_block = tpb;
    sp.n_chunks = n_chunks;
    for (uint32_t c = 0; c < NC && n_chunks; c++) {
      sp.out = in + (size_t)c * nq * n_chunks * slg::kVsSmallK;
      scan(c, true, dim3(qtiles, n_chunks));
    }
    select(0, NC, n_chunks * slg::kVsSmallK, n_chunks * slg::kVsSmallK, true);
  } else {
    const uint32_t tiles_per_chunk = chunk_docs / slg::kVsTileDocs;
    sp.out = in;
    sp.out_stride = chunk_docs;
    sp.tiles_per_block = 1;
    const uint32_t steps = std::max<uint32_t>((n_tiles + tiles_per_chunk - 1) / tiles_per_chunk, 1u);
    for (uint32_t s = 0; s < steps; s++) {
      const uint32_t t0 = s * tiles_per_chunk, t1 = std::min<uint32_t>(t0 + tiles_per_chunk, n_tiles);
      sp.tile_begin = t0;
      sp.tile_end = t1;
      for (uint32_t c = 0; c < NC; c++) {
        if (t1 > t0) scan(c, false, dim3(qtiles, t1 - t0));
        select(c, 1, (t1 > t0 ? t1 - t0 : 0) * slg::kVsTileDocs, chunk_docs, s + 1 == steps);
      }
    }
  }
  slg::VsBlendParams bp{};
  bp.dlist = dlist;
  bp.run_cnt = run_cnt;
  bp.nq = nq;
  bp.k = K;
  bp.n_clauses = NC;
  bp.alpha = a.alpha;
  for (uint32_t c = 0; c < NC; c++) bp.metric[c] = vc.metric[c];
  bp.doc_base = S.d_doc_base.as<uint32_t>();
  bp.n_segs = n_segs;
  bp.ukeys = ukeys;
  bp.P = P;
  bp.k_out = vc.k_out;
  bp.out_doc = a.out_doc;
  bp.out_seg = a.out_seg;
  bp.out_score = a.out_score;
  bp.out_vec = a.out_vec;
  bp.out_count = a.out_count;
  bp.out_total = a.out_total;
  launch_kernel_lds(slg::vs_blend_kernel<false>, bp, dim3(nq), slg::kVsSortThreads,
                   P > slg::kVsSortCap ? 0 : (size_t)P * 8, st);
}

void vs_device(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field, uint32_t cand_size,
               uint32_t k_out, const VsArgs &d) {
  VsCall vc;
  if (!vs_prepare(ix, nq, n_clauses, clause_field, cand_size, k_out, d, false, &vc)) return;
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  vs_run(ix, vc, d, ix->stream);
}

// host arrays: checks, pooled device buffers, H2D, the kernels, D2H and a wait, all on the index stream
// (Staging: slg_host.hpp)
void vs_staged(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field, uint32_t cand_size,
               uint32_t k_out, const VsArgs &h) {
  VsCall vc;
  if (!vs_prepare(ix, nq, n_clauses, clause_field, cand_size, k_out, h, true, &vc)) return;
  const size_t nqc = (size_t)nq * n_clauses, no = (size_t)nq * k_out;
  DeviceGuard g(ix->device);
  const hipStream_t st = ix->stream;
  Staging sg(&ix->pool, st);
  VsArgs d{};
  d.qvecs = sg.up(h.qvecs, (size_t)nq * vc.q_floats);
  d.alpha = sg.up(h.alpha, nqc);
  if (h.boost) d.boost = sg.up(h.boost, nqc);
  if (h.q_filter) d.q_filter = sg.up(h.q_filter, nq);
  d.out_doc = sg.up<uint32_t>(nullptr, no);
  d.out_seg = sg.up<uint32_t>(nullptr, no);
  d.out_score = sg.up<float>(nullptr, no);
  d.out_vec = sg.up<float>(nullptr, no);
  d.out_count = sg.up<uint32_t>(nullptr, nq);
  d.out_total = sg.up<uint64_t>(nullptr, nq);
  {
    std::lock_guard<std::mutex> lk(ix->mu);
    vs_run(ix, vc, d, st);
  }
  sg.down(h.out_doc, d.out_doc, no);
  sg.down(h.out_seg, d.out_seg, no);
  sg.down(h.out_score, d.out_score, no);
  sg.down(h.out_vec, d.out_vec, no);
  sg.down(h.out_count, d.out_count, nq);
  sg.down(h.out_total, d.out_total, nq);
  SLG_HIP(hipStreamSynchronize(st));
}
}  // namespace

size_t slghost::hy_work_layout(const VsCall &vc, uint32_t bm_k, void *base, HyWork *w) {
  const size_t n_run = (size_t)vc.n_clauses * vc.nq * vc.cand, n_cnt = (size_t)vc.n_clauses * vc.nq;
  const uint32_t P = slg::vs_pow2(vc.n_clauses * vc.cand + bm_k), Pb = slg::vs_pow2(std::max<uint32_t>(bm_k, 1u));
  // the union keys sort in LDS while they fit, and the BM25 hits behind them while both do
  const size_t n_u = P > slg::kVsSortCap ? (size_t)vc.nq * P : 0;
  const size_t n_b = P + Pb > slg::kVsSortCap ? (size_t)vc.nq * Pb : 0;
  if (w) {
    uint64_t *p = static_cast<uint64_t *>(base);
    w->run = p;
    w->dlist = w->run + n_run;
    w->ukeys = w->dlist + n_run;
    w->bkeys = w->ukeys + n_u;
    w->cnt = reinterpret_cast<uint32_t *>(w->bkeys + n_b);
    w->P = P;
    w->Pb = Pb;
  }
  return (2 * n_run + n_u + n_b) * 8 + 2 * n_cnt * 4 + 256;
}

void slghost::hy_fold(const VsCall &vc, const HyWork &w, const HyKeys &k, hipStream_t st) {
  const uint32_t K = vc.cand, NC = vc.n_clauses;
  const uint32_t fold_n = slg::kVsSortCap - K;  // keys of a pass: with the running list they sort in LDS
  slg::VsSelectParams sel{};
  sel.run = w.run;
  sel.run_cnt = w.cnt;
  sel.dlist = w.dlist;
  sel.nq = vc.nq;
  sel.k = K;
  sel.in = k.keys;
  sel.in_stride = (uint32_t)k.stride;
  sel.in_off = k.q_cand;
  sel.in_cnt = w.cnt + (size_t)NC * vc.nq;
  sel.in_base = k.slot_lo;
  sel.q0 = k.q_lo;
  sel.n_in = fold_n;
  const uint64_t passes = std::max<uint64_t>((k.max_cap + fold_n - 1) / fold_n, 1);
  const size_t lds = (size_t)slg::vs_pow2((uint32_t)std::min<uint64_t>(K + k.max_cap, slg::kVsSortCap)) * 8;
  for (uint64_t t = 0; t < passes; t++) {
    sel.in_skip = (uint32_t)(t * fold_n);
    sel.final_ = t + 1 == passes ? 1u : 0u;
    launch_kernel_lds(slg::vs_select_kernel, sel, dim3(k.q_hi - k.q_lo, NC), slg::kVsSortThreads, lds, st);
  }
}

void slghost::hy_blend(const VsCall &vc, const VsArgs &a, const HyWork &w, const uint32_t *bm_doc,
                       const uint32_t *bm_seg, const float *bm_score, const uint32_t *bm_count, uint32_t bm_k,
                       hipStream_t st) {
  const IndexState &S = *vc.S;
  slg::VsBlendParams bp{};
  bp.dlist = w.dlist;
  bp.run_cnt = w.cnt;
  bp.nq = vc.nq;
  bp.k = vc.cand;
  bp.n_clauses = vc.n_clauses;
  bp.alpha = a.alpha;
  for (uint32_t c = 0; c < vc.n_clauses; c++) bp.metric[c] = vc.metric[c];
  bp.doc_base = S.d_doc_base.as<uint32_t>();
  bp.n_segs = (uint32_t)S.segs.size();
  bp.ukeys = w.ukeys;
  bp.P = w.P;
  bp.k_out = vc.k_out;
  bp.out_doc = a.out_doc;
  bp.out_seg = a.out_seg;
  bp.out_score = a.out_score;
  bp.out_vec = a.out_vec;
  bp.out_count = a.out_count;
  bp.out_total = a.out_total;
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
  return guarded([&] {
    vs_staged(ix, nq, n_clauses, clause_field, cand_size, k_out,
              {qvecs, alpha, boost, q_filter, out_doc, out_seg, out_score, out_vec_score, out_count, out_total});
  });
}

int slg_vector_search_batch_device(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                                   const float *d_qvecs, const float *d_alpha, const float *d_boost,
                                   const int32_t *d_q_filter, uint32_t cand_size, uint32_t k_out,
                                   uint32_t *d_out_doc, uint32_t *d_out_seg, float *d_out_score,
                                   float *d_out_vec_score, uint32_t *d_out_count, uint64_t *d_out_total) {
  return guarded([&] {
    vs_device(ix, nq, n_clauses, clause_field, cand_size, k_out,
              {d_qvecs, d_alpha, d_boost, d_q_filter, d_out_doc, d_out_seg, d_out_score, d_out_vec_score,
               d_out_count, d_out_total});
  });
}

}  // extern "C"
