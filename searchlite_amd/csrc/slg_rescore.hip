// slg_rescore.hip — rescore batches (slg_batch_prepare_rescore): the planned term table onto the device, the
// launch of rescore_kernel behind the batch's first pass, and slg_batch_fetch_rescore.  (The checks of a spec
// and the table itself: slg_plan.cpp, check_rescore / plan_rescore.)
#include "slg_host.hpp"

#include "slg_rescore.hpp"

using namespace slghost;

static_assert(sizeof(slg::RescoreTerm) == 24 && sizeof(slg::RescoreQuery) == 32, "the table is copied in 8-byte words");

void slghost::rescore_attach(slg_batch *b, const slgplan::RescorePlan &rp) {
  slg_index *ix = b->idx;
  b->rescore = true;
  b->rs_lds_rows = (std::max(rp.max_window, 2u) + 1u) & ~1u;  // even: the table behind the rows stays 8-byte aligned
  b->rs_max_table = rp.max_table;
  upload_image(b->d_rs_desc, &ix->pool, {image_part(rp.queries), image_part(rp.terms)});
  b->d_rs_side.alloc_pooled(&ix->pool, 3 * (size_t)b->nq * b->k * 4);
}

void slghost::rescore_launch(slg_batch *b, hipStream_t st) {
  if (b->nq == 0 || b->k == 0) return;
  const IndexState &S = *b->snap;
  slg::RescoreParams p{};
  p.segs = S.d_segs.as<slg::SegDev>();
  p.n_segs = (uint32_t)S.segs.size();
  p.queries = b->d_rs_desc.as<const slg::RescoreQuery>();
  p.terms = reinterpret_cast<const slg::RescoreTerm *>(b->d_rs_desc.as<unsigned char>() +
                                                       (size_t)b->nq * sizeof(slg::RescoreQuery));
  p.out_doc = b->d_out_doc;
  p.out_seg = b->d_out_seg;
  p.out_score = b->d_out_score;
  p.out_count = b->d_out_count;
  const size_t n = (size_t)b->nq * b->k;
  p.first_score = b->d_rs_side.as<float>();
  p.rescore_score = p.first_score + n;
  p.rescored = b->d_rs_side.as<uint32_t>() + 2 * n;
  p.nq = b->nq;
  p.k = b->k;
  p.lds_rows = b->rs_lds_rows;
  SLG_HIP(slg::launch_rescore(p, kregs_for(b->rs_lds_rows), slg::rescore_lds_bytes(b->rs_lds_rows, b->rs_max_table), st));
}

extern "C" {

int slg_batch_fetch_rescore(slg_batch *b, float *out_first_score, float *out_rescore_score, uint32_t *out_rescored) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->rescore, "not a rescore batch (slg_batch_prepare_rescore)");
    SLG_REQUIRE(b->launched, "the batch has not run");
    DeviceGuard g(b->idx->device);
    const hipStream_t st = locked_stream(b);
    const size_t n = (size_t)b->nq * b->k;
    const float *side = b->d_rs_side.as<const float>();
    void *const dst[3] = {out_first_score, out_rescore_score, out_rescored};
    for (int i = 0; i < 3; i++)
      if (n && dst[i]) SLG_HIP(hipMemcpyAsync(dst[i], side + i * n, n * 4, hipMemcpyDeviceToHost, st));
    SLG_HIP(wait_stream(st));
  });
}

}  // extern "C"
