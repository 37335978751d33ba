// slg_rerank.hip — the vector rerank entry points (slg_rerank_*; kernels: slg_rerank.hpp).
#include "slg_host.hpp"

#include "slg_rerank.hpp"

using namespace slghost;

// (what it answers: slg_host.hpp)
void slghost::field_facts(const IndexState &S, uint32_t f, uint32_t *dim, int32_t *metric,
                          const slg::VecSegDev **vsegs, bool mixed_metric) {
  if (f == 0) {
    uint32_t d = 0;
    int32_t m = -1;
    for (auto &s : S.segs) {
      if (!s->store->vec_dim) continue;
      SLG_REQUIRE(d == 0 || d == s->store->vec_dim, "segments disagree on vec_dim");
      SLG_REQUIRE(mixed_metric || m < 0 || m == s->store->vec_metric, "segments disagree on the vector metric");
      d = s->store->vec_dim;
      m = s->store->vec_metric;
    }
    if (d == 0) throw SlgError(SLG_ERR_UNSUPPORTED, "index has no vector field");
    *dim = d;
    *metric = m;
    *vsegs = S.d_vsegs.as<slg::VecSegDev>();
    return;
  }
  SLG_REQUIRE(f <= S.vfields.size(), "unknown vector field id");
  const VecFieldHost &vf = *S.vfields[f - 1];
  *dim = vf.dim;
  *metric = vf.metric;
  *vsegs = vf.d_vsegs.as<slg::VecSegDev>();
}

extern "C" {

namespace {
enum class RerankShape { One, Multi, Fields };  // rerank_kernel, rerank_multi_kernel, rerank_fields_kernel

// One rerank call, checked against one snapshot of the index.  fp holds the parameters of every
// shape (the fields kernel's are a superset): base, boost, n_clauses, q_floats = the floats of one
// query's clause vectors; the per-clause tables are the fields shape's only.
struct RerankCall {
  std::shared_ptr<const IndexState> S;  // (a retired state waits for the device before its tables go)
  RerankShape shape = RerankShape::One;
  slg::RerankFieldsParams fp{};
};

// The host-only step of every rerank entry: all checks, in one order for the host and device forms,
// then the kernel facts of the call's shape.  io's pointers are only tested for NULL (mem names
// their memory in the message).  false: nq == 0, nothing to do.  Multi-clause entries with one
// clause and no boost take the single-clause kernel, which has no n_clauses check.
bool rerank_prepare(slg_index *ix, bool fields, uint32_t n_clauses, const uint32_t *clause_field, const float *boost,
                    const slg::RerankParams &io, const char *mem, RerankCall *rc) {
  if (fields)
    SLG_REQUIRE(ix != nullptr && clause_field != nullptr, "index or clause_field is NULL");
  else
    SLG_REQUIRE(ix != nullptr, "index is NULL");
  rc->shape = fields ? RerankShape::Fields
                     : (n_clauses == 1 && boost == nullptr ? RerankShape::One : RerankShape::Multi);
  if (rc->shape != RerankShape::One && (n_clauses < 1 || n_clauses > SLG_MAX_VECTOR_CLAUSES))
    throw SlgError(SLG_ERR_UNSUPPORTED, "n_clauses outside 1..SLG_MAX_VECTOR_CLAUSES");
  if (io.k_out > SLG_MAX_RERANK_K) throw SlgError(SLG_ERR_UNSUPPORTED, "k_out > SLG_MAX_RERANK_K");
  if (io.nq == 0) return false;
  SLG_REQUIRE(io.qvecs && io.alpha && io.cand_count && io.out_count, std::string(mem) + " arrays are NULL");
  SLG_REQUIRE(io.max_cand == 0 || (io.cand_doc && io.cand_seg && io.cand_bm25), "candidate arrays are NULL");
  SLG_REQUIRE(io.k_out == 0 || (io.out_doc && io.out_seg && io.out_score), "output arrays are NULL");
  rc->S = ix->snapshot();
  const IndexState &S = *rc->S;
  slg::RerankFieldsParams &fp = rc->fp;
  fp.base = io;
  fp.base.n_segs = (uint32_t)S.segs.size();
  fp.boost = boost;
  fp.n_clauses = n_clauses;
  if (rc->shape == RerankShape::Fields) {
    for (uint32_t c = 0; c < n_clauses; c++) {
      field_facts(S, clause_field[c], &fp.cdim[c], &fp.cmetric[c], &fp.cvsegs[c]);
      fp.coff[c] = fp.q_floats;
      fp.q_floats += fp.cdim[c];
    }
    if (slg::rerank_fields_lds_floats(n_clauses, fp.q_floats, io.max_cand) > slg::kRerankMultiLdsFloats)
      throw SlgError(SLG_ERR_UNSUPPORTED, "clause vectors + n_clauses * max_cand exceed the LDS budget of the rerank");
    return true;
  }
  int32_t metric;
  field_facts(S, 0, &fp.base.dim, &metric, &fp.base.vsegs, rc->shape == RerankShape::One);
  fp.base.metric = metric;
  fp.q_floats = n_clauses * fp.base.dim;
  if (rc->shape == RerankShape::One) {
    if (io.max_cand > slg::kRerankMaxCand)
      throw SlgError(SLG_ERR_UNSUPPORTED, "max_cand > " + std::to_string(slg::kRerankMaxCand));
    return true;
  }
  for (auto &s : S.segs)
    if (!s->store->vec_dim) throw SlgError(SLG_ERR_UNSUPPORTED, "multi-clause rerank needs the vector field in every segment");
  if (slg::rerank_multi_lds_floats(n_clauses, fp.base.dim, io.max_cand) > slg::kRerankMultiLdsFloats)
    throw SlgError(SLG_ERR_UNSUPPORTED, "n_clauses * (dim + max_cand) exceeds the LDS budget of the multi-clause rerank");
  return true;
}

// The launch step: the kernel of the call's shape on st, with the device pointers of rc.fp (the
// caller holds ix->mu and the device)
void rerank_launch(const RerankCall &rc, hipStream_t st) {
  const slg::RerankFieldsParams &fp = rc.fp;
  const int kregs = kregs_for(fp.base.k_out ? fp.base.k_out : 1);
  if (rc.shape == RerankShape::One) {
    SLG_HIP(slg::launch_rerank(fp.base, kregs, st));
  } else if (rc.shape == RerankShape::Multi) {
    const slg::RerankMultiParams mp{fp.base, fp.boost, fp.n_clauses, fp.base.dim + 4};
    SLG_HIP(slg::launch_rerank_multi(mp, kregs, st));
  } else {
    SLG_HIP(slg::launch_rerank_fields(fp, kregs, st));
  }
}

// The _device entries: device arrays in and out, asynchronous on the index stream or, b set, on the
// batch's (read under ix->mu, with the launch)
void rerank_device(slg_index *ix, const slg_batch *b, bool fields, uint32_t n_clauses, const uint32_t *clause_field,
                   const float *d_boost, const slg::RerankParams &d) {
  RerankCall rc;
  if (!rerank_prepare(ix, fields, n_clauses, clause_field, d_boost, d, "device", &rc)) return;
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  rerank_launch(rc, b ? batch_stream(b) : ix->stream);
}

// The host-array entries: checks first, then pooled device buffers, H2D, launch, D2H and a wait, all on
// the index stream (Staging: slg_host.hpp)
void rerank_staged(slg_index *ix, bool fields, uint32_t n_clauses, const uint32_t *clause_field, const float *boost,
                   const slg::RerankParams &h) {
  RerankCall rc;
  if (!rerank_prepare(ix, fields, n_clauses, clause_field, boost, h, "host", &rc)) return;
  const size_t nq = h.nq, nqc = nq * n_clauses, nc = nq * h.max_cand, no = nq * h.k_out;
  DeviceGuard g(ix->device);
  const hipStream_t st = ix->stream;
  Staging sg(&ix->pool, st);
  slg::RerankParams &d = rc.fp.base;
  d.qvecs = sg.up(h.qvecs, nq * rc.fp.q_floats);
  d.alpha = sg.up(h.alpha, nqc);
  if (boost) rc.fp.boost = sg.up(boost, nqc);
  d.cand_doc = sg.up(h.cand_doc, nc);
  d.cand_seg = sg.up(h.cand_seg, nc);
  d.cand_bm25 = sg.up(h.cand_bm25, nc);
  d.cand_count = sg.up(h.cand_count, nq);
  d.out_doc = sg.up<uint32_t>(nullptr, no);
  d.out_seg = sg.up<uint32_t>(nullptr, no);
  d.out_score = sg.up<float>(nullptr, no);
  d.out_vec = sg.up<float>(nullptr, no);
  d.out_count = sg.up<uint32_t>(nullptr, nq);
  {
    std::lock_guard<std::mutex> lk(ix->mu);
    rerank_launch(rc, st);
  }
  sg.down(h.out_doc, d.out_doc, no);
  sg.down(h.out_seg, d.out_seg, no);
  sg.down(h.out_score, d.out_score, no);
  sg.down(h.out_vec, d.out_vec, no);
  sg.down(h.out_count, d.out_count, nq);
  SLG_HIP(hipStreamSynchronize(st));
}
}  // namespace

int slg_rerank_batch_device(slg_index *ix, uint32_t nq, const float *d_qvecs, const float *d_alpha,
                            const uint32_t *d_cand_doc, const uint32_t *d_cand_seg,
                            const float *d_cand_bm25, const uint32_t *d_cand_count,
                            uint32_t max_cand, uint32_t k_out, uint32_t *d_out_doc,
                            uint32_t *d_out_seg, float *d_out_score, float *d_out_vec_score,
                            uint32_t *d_out_count) {
  return slg_rerank_multi_batch_device(ix, nq, 1, d_qvecs, d_alpha, nullptr, d_cand_doc, d_cand_seg, d_cand_bm25,
                                       d_cand_count, max_cand, k_out, d_out_doc, d_out_seg, d_out_score,
                                       d_out_vec_score, d_out_count);
}

int slg_rerank_multi_batch_device(slg_index *ix, uint32_t nq, uint32_t n_clauses, const float *d_qvecs,
                                  const float *d_alpha, const float *d_boost, const uint32_t *d_cand_doc,
                                  const uint32_t *d_cand_seg, const float *d_cand_bm25,
                                  const uint32_t *d_cand_count, uint32_t max_cand, uint32_t k_out,
                                  uint32_t *d_out_doc, uint32_t *d_out_seg, float *d_out_score,
                                  float *d_out_vec_score, uint32_t *d_out_count) {
  return guarded([&] {
    rerank_device(ix, nullptr, false, n_clauses, nullptr, d_boost,
                  {nullptr, 0, 0, d_qvecs, d_alpha, d_cand_doc, d_cand_seg, d_cand_bm25, d_cand_count, max_cand,
                   k_out, d_out_doc, d_out_seg, d_out_score, d_out_vec_score, d_out_count, nq});
  });
}

int slg_batch_rerank_device(slg_batch *b, uint32_t n_clauses, const float *d_qvecs, const float *d_alpha,
                            const float *d_boost, uint32_t k_out, uint32_t *d_out_doc, uint32_t *d_out_seg,
                            float *d_out_score, float *d_out_vec_score, uint32_t *d_out_count) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    rerank_device(b->idx, b, false, n_clauses, nullptr, d_boost,
                  {nullptr, 0, 0, d_qvecs, d_alpha, b->d_out_doc, b->d_out_seg, b->d_out_score, b->d_out_count,
                   b->k, k_out, d_out_doc, d_out_seg, d_out_score, d_out_vec_score, d_out_count, b->nq});
  });
}

int slg_rerank_fields_batch_device(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                                   const float *d_qvecs, const float *d_alpha, const float *d_boost,
                                   const uint32_t *d_cand_doc, const uint32_t *d_cand_seg,
                                   const float *d_cand_bm25, const uint32_t *d_cand_count, uint32_t max_cand,
                                   uint32_t k_out, uint32_t *d_out_doc, uint32_t *d_out_seg, float *d_out_score,
                                   float *d_out_vec_score, uint32_t *d_out_count) {
  return guarded([&] {
    rerank_device(ix, nullptr, true, n_clauses, clause_field, d_boost,
                  {nullptr, 0, 0, d_qvecs, d_alpha, d_cand_doc, d_cand_seg, d_cand_bm25, d_cand_count, max_cand,
                   k_out, d_out_doc, d_out_seg, d_out_score, d_out_vec_score, d_out_count, nq});
  });
}

int slg_rerank_fields_batch(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                            const float *qvecs, const float *alpha, const float *boost,
                            const uint32_t *cand_doc, const uint32_t *cand_seg, const float *cand_bm25,
                            const uint32_t *cand_count, uint32_t max_cand, uint32_t k_out, uint32_t *out_doc,
                            uint32_t *out_seg, float *out_score, float *out_vec_score, uint32_t *out_count) {
  return guarded([&] {
    rerank_staged(ix, true, n_clauses, clause_field, boost,
                  {nullptr, 0, 0, qvecs, alpha, cand_doc, cand_seg, cand_bm25, cand_count, max_cand, k_out, out_doc,
                   out_seg, out_score, out_vec_score, out_count, nq});
  });
}

int slg_rerank_multi_batch(slg_index *ix, uint32_t nq, uint32_t n_clauses, const float *qvecs,
                           const float *alpha, const float *boost, const uint32_t *cand_doc,
                           const uint32_t *cand_seg, const float *cand_bm25, const uint32_t *cand_count,
                           uint32_t max_cand, uint32_t k_out, uint32_t *out_doc, uint32_t *out_seg,
                           float *out_score, float *out_vec_score, uint32_t *out_count) {
  return guarded([&] {
    rerank_staged(ix, false, n_clauses, nullptr, boost,
                  {nullptr, 0, 0, qvecs, alpha, cand_doc, cand_seg, cand_bm25, cand_count, max_cand, k_out, out_doc,
                   out_seg, out_score, out_vec_score, out_count, nq});
  });
}

int slg_rerank_batch(slg_index *ix, uint32_t nq, const float *qvecs, const float *alpha,
                     const uint32_t *cand_doc, const uint32_t *cand_seg, const float *cand_bm25,
                     const uint32_t *cand_count, uint32_t max_cand, uint32_t k_out,
                     uint32_t *out_doc, uint32_t *out_seg, float *out_score, float *out_vec_score,
                     uint32_t *out_count) {
  return slg_rerank_multi_batch(ix, nq, 1, qvecs, alpha, nullptr, cand_doc, cand_seg, cand_bm25, cand_count,
                                max_cand, k_out, out_doc, out_seg, out_score, out_vec_score, out_count);
}

}  // extern "C"
