// slg_bool.hip — bool batches (slg_batch_prepare_bool): the planned clause tables onto the device and the launch
// of bool_filter_kernel between the batch's scoring kernel and its select.  (The checks of a spec and the tables
// themselves: slg_plan.cpp, check_bool / plan_bool.)
#include "slg_host.hpp"

#include "slg_bool.hpp"

using namespace slghost;

static_assert(sizeof(slg::BoolTerm) == 16 && sizeof(slg::BoolQuery) == 32, "the tables are read in whole words, terms 16-byte aligned");

void slghost::bool_attach(slg_batch *b, const slgplan::BoolPlan &bp) {
  slg_index *ix = b->idx;
  b->boolean = true;
  b->bool_groups = bp.n_groups;
  const size_t q_bytes = bp.queries.size() * sizeof(slg::BoolQuery), t_bytes = bp.terms.size() * sizeof(slg::BoolTerm);
  std::vector<unsigned char> image(q_bytes + t_bytes);
  if (q_bytes) std::memcpy(image.data(), bp.queries.data(), q_bytes);
  if (t_bytes) std::memcpy(image.data() + q_bytes, bp.terms.data(), t_bytes);
  b->d_bool_desc.alloc_pooled(&ix->pool, image.size());
  if (!image.empty()) SLG_HIP(hipMemcpy(b->d_bool_desc.p, image.data(), image.size(), hipMemcpyHostToDevice));
}

void slghost::bool_launch(slg_batch *b, hipStream_t st) {
  if (b->n_slices == 0 || b->bool_groups == 0) return;  // nothing was scored, or no query has a clause table
  if (!b->cand_mode) throw SlgError(SLG_ERR_INTERNAL, "a bool batch was not planned in candidates mode");
  const IndexState &S = *b->snap;
  slg::BoolFilterParams p{};
  p.segs = S.d_segs.as<slg::SegDev>();
  p.sq = b->d_sq;
  p.slice_sq = b->d_slice_sq;
  p.queries = b->d_bool_desc.as<const slg::BoolQuery>();
  p.terms = reinterpret_cast<const slg::BoolTerm *>(b->d_bool_desc.as<unsigned char>() +
                                                    (size_t)b->nq * sizeof(slg::BoolQuery));
  p.cand = b->d_cand.as<uint2>();
  p.slice_cbeg = b->d_slice_cbeg.as<uint64_t>();
  p.slice_ccnt = b->d_slice_ccnt.as<uint32_t>();
  p.q_scored = b->d_q_scored.as<uint32_t>();
  p.n_slices = b->n_slices;
  p.n_segs = (uint32_t)S.segs.size();
  constexpr uint32_t per_block = slg::kBoolThreads / 64;
  hipLaunchKernelGGL(slg::bool_filter_kernel, dim3((b->n_slices + per_block - 1) / per_block), dim3(slg::kBoolThreads),
                     0, st, p);
  SLG_HIP(hipGetLastError());
}
