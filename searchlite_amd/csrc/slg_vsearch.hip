// slg_vsearch.hip — exact vector-only search (slg_vector_search_batch*; kernels: slg_vsearch.hpp) and the two-pass
// search over a bf16 copy of the store (slg_vector_search_batch_approx*; kernels: slg_vsearch_approx.hpp).
#include "slg_host.hpp"

#include "slg_vsearch.hpp"
#include "slg_vsearch_approx.hpp"

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
    // one round of resident workgroups: as many as the LDS of a CU holds (at most 3, the VGPR bound; 2 for
    // vs_scan_bf16_kernel, whose 197 registers leave two waves per SIMD)
    int n_cu = 0;
    SLG_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ix->device));
    const uint32_t per_cu = std::min<uint32_t>(bf16 ? 2u : 3u, (uint32_t)((160u << 10) / pl.lds(true)));
    const uint32_t target = std::max<uint32_t>((uint32_t)n_cu, 1u) * std::max<uint32_t>(per_cu, 1u);
    pl.n_chunks = std::min<uint32_t>(std::max<uint32_t>((target + pl.qtiles - 1) / pl.qtiles, 1u),
                                     std::min<uint32_t>(n_tiles, (slg::kVsSortCap - slg::kVsSmallK) / slg::kVsSmallK));
    pl.tpb = (pl.n_tiles + pl.n_chunks - 1) / pl.n_chunks;
    pl.n_chunks = (pl.n_tiles + pl.tpb - 1) / pl.tpb;
  } else if (!pl.small) {
    pl.chunk_docs = ((slg::kVsSortCap - K) / slg::kVsTileDocs) * slg::kVsTileDocs;
  }
  pl.n_in = pl.small ? (size_t)vc.n_clauses * vc.nq * pl.n_chunks * slg::kVsSmallK : (size_t)vc.nq * pl.chunk_docs;
  return pl;
}

void vs_select(uint64_t *run, uint32_t *run_cnt, uint64_t *dlist, const uint64_t *in, uint32_t nq, uint32_t K,
               uint32_t c0, uint32_t n_cl, uint32_t n_in_q, uint32_t stride, bool final_, hipStream_t st) {
  slg::VsSelectParams sel{};
  sel.run = run;
  sel.run_cnt = run_cnt;
  sel.dlist = dlist;
  sel.nq = nq;
  sel.k = K;
  sel.in = in;
  sel.c0 = c0;
  sel.n_in = n_in_q;
  sel.in_stride = stride;
  sel.final_ = final_ ? 1u : 0u;
  const size_t lds = (size_t)slg::vs_pow2(K + n_in_q) * 8;
  launch_kernel_lds(slg::vs_select_kernel, sel, dim3(nq, n_cl), slg::kVsSortThreads, lds, st);
}

// the clause lists of one call on st: per (clause, query) the best K keys in run (best first, run_cnt of them;
// zeroed by the caller) and, final_, sorted by doc in dlist.  The exact scan, or (pl.bf16) the scan of the bf16 copies
void vs_lists(const VsCall &vc, const VsArgs &a, const VsPlan &pl, uint32_t K, uint64_t *run, uint32_t *run_cnt,
              uint64_t *dlist, uint64_t *in, bool final_, hipStream_t st) {
  const IndexState &S = *vc.S;
  const uint32_t nq = vc.nq, NC = vc.n_clauses;
  slg::VsScanBf16Params bp{};
  slg::VsScanParams &sp = bp.s;
  sp.segs = S.d_segs.as<slg::SegDev>();
  sp.reject_table = S.d_reject_table.as<const uint32_t *>();
  sp.doc_base = S.d_doc_base.as<uint32_t>();
  sp.n_segs = (uint32_t)S.segs.size();
  sp.n_filters = (uint32_t)S.filters.size();
  sp.nq = nq;
  sp.qvecs = a.qvecs;
  sp.q_stride = vc.q_floats;
  sp.boost = a.boost;
  sp.n_clauses = NC;
  sp.q_filter = a.q_filter;
  sp.k = K;
  sp.cap = pl.cap;
  auto scan = [&](uint32_t c, bool topk, dim3 grid) {
    sp.vsegs = vc.vsegs[c];
    bp.csegs = vc.csegs[c];
    sp.dim = vc.dim[c];
    sp.q_off = vc.coff[c];
    sp.clause = c;
    sp.qvec4 = (vc.q_floats % 4 == 0 && vc.coff[c] % 4 == 0 && ((uintptr_t)a.qvecs & 15) == 0) ? 1u : 0u;
    const size_t lds = pl.lds(topk);
    const bool cosine = vc.metric[c] == 0;
    if (pl.bf16) {
      if (cosine)
        topk ? launch_kernel_lds(slg::vs_scan_bf16_kernel<0, true>, bp, grid, 256, lds, st)
             : launch_kernel_lds(slg::vs_scan_bf16_kernel<0, false>, bp, grid, 256, lds, st);
      else
        topk ? launch_kernel_lds(slg::vs_scan_bf16_kernel<1, true>, bp, grid, 256, lds, st)
             : launch_kernel_lds(slg::vs_scan_bf16_kernel<1, false>, bp, grid, 256, lds, st);
    } else if (cosine) {
      topk ? launch_kernel_lds(slg::vs_scan_kernel<0, true>, sp, grid, 256, lds, st)
           : launch_kernel_lds(slg::vs_scan_kernel<0, false>, sp, grid, 256, lds, st);
    } else {
      topk ? launch_kernel_lds(slg::vs_scan_kernel<1, true>, sp, grid, 256, lds, st)
           : launch_kernel_lds(slg::vs_scan_kernel<1, false>, sp, grid, 256, lds, st);
    }
  };
  if (pl.small) {
    sp.tile_begin = 0;
    sp.tile_end = pl.n_tiles;
    sp.tiles_per_block = pl.tpb;
    sp.n_chunks = pl.n_chunks;
    for (uint32_t c = 0; c < NC && pl.n_chunks; c++) {
      sp.out = in + (size_t)c * nq * pl.n_chunks * slg::kVsSmallK;
      scan(c, true, dim3(pl.qtiles, pl.n_chunks));
    }
    vs_select(run, run_cnt, dlist, in, nq, K, 0, NC, pl.n_chunks * slg::kVsSmallK, pl.n_chunks * slg::kVsSmallK,
              final_, st);
  } else {
    const uint32_t tiles_per_chunk = pl.chunk_docs / slg::kVsTileDocs;
    sp.out = in;
    sp.out_stride = pl.chunk_docs;
    sp.tiles_per_block = 1;
    const uint32_t steps = std::max<uint32_t>((pl.n_tiles + tiles_per_chunk - 1) / tiles_per_chunk, 1u);
    for (uint32_t s = 0; s < steps; s++) {
      const uint32_t t0 = s * tiles_per_chunk, t1 = std::min<uint32_t>(t0 + tiles_per_chunk, pl.n_tiles);
      sp.tile_begin = t0;
      sp.tile_end = t1;
      for (uint32_t c = 0; c < NC; c++) {
        if (t1 > t0) scan(c, false, dim3(pl.qtiles, t1 - t0));
        vs_select(run, run_cnt, dlist, in, nq, K, c, 1, (t1 > t0 ? t1 - t0 : 0) * slg::kVsTileDocs, pl.chunk_docs,
                  final_ && s + 1 == steps, st);
      }
    }
  }
}

// union of the clause lists (K keys each, sorted by doc), blend, top k_out
void vs_blend(const VsCall &vc, const VsArgs &a, const uint64_t *dlist, const uint32_t *run_cnt, uint32_t K,
              uint64_t *ukeys, uint32_t P, hipStream_t st) {
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
  launch_kernel_lds(slg::vs_blend_kernel<false>, bp, dim3(vc.nq), slg::kVsSortThreads,
                   P > slg::kVsSortCap ? 0 : (size_t)P * 8, st);
}

// the kernels of one call on st, device arrays in a (the caller holds ix->mu and the device).  refine 0: the exact
// search; else the two-pass one: lists of `refine` keys from the bf16 copies, their exact scores, the best cand_size
void vs_run(slg_index *ix, const VsCall &vc, const VsArgs &a, uint32_t refine, hipStream_t st) {
  const uint32_t nq = vc.nq, NC = vc.n_clauses, K = vc.cand, R = refine ? refine : K;
  const VsPlan pl = vs_plan(ix, vc, R, refine != 0);
  const size_t n_run = (size_t)NC * nq * K, n_first = refine ? (size_t)NC * nq * R : 0, n_cnt = (size_t)NC * nq;
  const uint32_t P = slg::vs_pow2(NC * K);
  const size_t n_u = P > slg::kVsSortCap ? (size_t)nq * P : 0;
  const size_t bytes = (2 * n_run + n_first + std::max<size_t>(pl.n_in, 1) + n_u) * 8 + 2 * n_cnt * 4 + 256;
  if (ix->vs_scratch.bytes < bytes) ix->vs_scratch.alloc(bytes + bytes / 4, &ix->pool);
  uint64_t *run = ix->vs_scratch.as<uint64_t>(), *dlist = run + n_run, *first = dlist + n_run;
  uint64_t *in = first + n_first, *ukeys = in + std::max<size_t>(pl.n_in, 1);
  uint32_t *run_cnt = reinterpret_cast<uint32_t *>(ukeys + n_u), *first_cnt = run_cnt + n_cnt;
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
      rp.qvec4 = (vc.q_floats % 4 == 0 && vc.coff[c] % 4 == 0 && ((uintptr_t)a.qvecs & 15) == 0) ? 1u : 0u;
      rp.clause = c;
      if (vc.metric[c] == 0)
        hipLaunchKernelGGL(slg::vs_refine_kernel<0>, dim3(nq), dim3(256), 0, st, rp);
      else
        hipLaunchKernelGGL(slg::vs_refine_kernel<1>, dim3(nq), dim3(256), 0, st, rp);
      SLG_HIP(hipGetLastError());
    }
    // the refined keys fold into the final lists in passes that sort in LDS with the running list
    const uint32_t fold_n = slg::kVsSortCap - K;
    for (uint32_t o = 0; o < R; o += fold_n)
      vs_select(run, run_cnt, dlist, first + o, nq, K, 0, NC, std::min(fold_n, R - o), R, o + fold_n >= R, st);
  }
  vs_blend(vc, a, dlist, run_cnt, K, ukeys, P, st);
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
void vs_check_refine(uint32_t cand_size, uint32_t refine) {
  if (refine < cand_size || refine > SLG_MAX_VECTOR_CANDIDATES)
    throw SlgError(SLG_ERR_UNSUPPORTED, "refine outside cand_size..SLG_MAX_VECTOR_CANDIDATES");
}

// refine 0: the exact search (both forms)
void vs_device(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field, uint32_t cand_size,
               uint32_t refine, uint32_t k_out, const VsArgs &d) {
  VsCall vc;
  if (!vs_prepare(ix, nq, n_clauses, clause_field, cand_size, k_out, d, false, &vc)) return;
  if (refine) vs_prepare_approx(n_clauses, clause_field, &vc);
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  vs_run(ix, vc, d, refine, ix->stream);
}

// host arrays: checks, pooled device buffers, H2D, the kernels, D2H and a wait, all on the index stream
// (Staging: slg_host.hpp)
void vs_staged(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field, uint32_t cand_size,
               uint32_t refine, uint32_t k_out, const VsArgs &h) {
  VsCall vc;
  if (!vs_prepare(ix, nq, n_clauses, clause_field, cand_size, k_out, h, true, &vc)) return;
  if (refine) vs_prepare_approx(n_clauses, clause_field, &vc);
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
    vs_run(ix, vc, d, refine, st);
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
    vs_staged(ix, nq, n_clauses, clause_field, cand_size, 0, k_out,
              {qvecs, alpha, boost, q_filter, out_doc, out_seg, out_score, out_vec_score, out_count, out_total});
  });
}

int slg_vector_search_batch_device(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                                   const float *d_qvecs, const float *d_alpha, const float *d_boost,
                                   const int32_t *d_q_filter, uint32_t cand_size, uint32_t k_out,
                                   uint32_t *d_out_doc, uint32_t *d_out_seg, float *d_out_score,
                                   float *d_out_vec_score, uint32_t *d_out_count, uint64_t *d_out_total) {
  return guarded([&] {
    vs_device(ix, nq, n_clauses, clause_field, cand_size, 0, k_out,
              {d_qvecs, d_alpha, d_boost, d_q_filter, d_out_doc, d_out_seg, d_out_score, d_out_vec_score,
               d_out_count, d_out_total});
  });
}

int slg_vector_search_batch_approx(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                                   const float *qvecs, const float *alpha, const float *boost, const int32_t *q_filter,
                                   uint32_t cand_size, uint32_t refine, uint32_t k_out, uint32_t *out_doc,
                                   uint32_t *out_seg, float *out_score, float *out_vec_score, uint32_t *out_count,
                                   uint64_t *out_total) {
  return guarded([&] {
    vs_check_refine(cand_size, refine);
    vs_staged(ix, nq, n_clauses, clause_field, cand_size, refine, k_out,
              {qvecs, alpha, boost, q_filter, out_doc, out_seg, out_score, out_vec_score, out_count, out_total});
  });
}

int slg_vector_search_batch_approx_device(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                                          const float *d_qvecs, const float *d_alpha, const float *d_boost,
                                          const int32_t *d_q_filter, uint32_t cand_size, uint32_t refine,
                                          uint32_t k_out, uint32_t *d_out_doc, uint32_t *d_out_seg,
                                          float *d_out_score, float *d_out_vec_score, uint32_t *d_out_count,
                                          uint64_t *d_out_total) {
  return guarded([&] {
    vs_check_refine(cand_size, refine);
    vs_device(ix, nq, n_clauses, clause_field, cand_size, refine, k_out,
              {d_qvecs, d_alpha, d_boost, d_q_filter, d_out_doc, d_out_seg, d_out_score, d_out_vec_score,
               d_out_count, d_out_total});
  });
}

}  // extern "C"
