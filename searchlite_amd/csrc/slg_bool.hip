// slg_bool.hip — bool batches (slg_batch_prepare_bool): the planned clause tables onto the device and the launch
// of bool_filter_kernel between the batch's scoring kernel and its select.  (The checks of a spec and the tables
// themselves: slg_plan.cpp, check_bool / plan_bool.)
#include "slg_host.hpp"

#include "slg_bool.hpp"

using namespace slghost;

static_assert(sizeof(slg::BoolTerm) == 16 && sizeof(slg::BoolQuery) == 32, "the tables are read in whole words, terms 16-byte aligned");

void slghost::bool_attach(slg_batch *b, const slgplan::BoolPlan &bp) {
  b->boolean = true;
  b->bool_groups = bp.n_groups;
  upload_image(b->d_bool_desc, &b->idx->pool, {image_part(bp.queries), image_part(bp.terms)});
}

void slghost::bool_launch(slg_batch *b, hipStream_t st) {
  if (b->n_slices == 0 || b->bool_groups == 0) return;  // nothing was scored, or no query has a clause table
  if (!b->cand_mode) throw SlgError(SLG_ERR_INTERNAL, "a bool batch was not planned in candidates mode");
  slg::BoolFilterParams p{};
  fill_clause_filter(p, b);
  constexpr uint32_t per_block = slg::kBoolThreads / 64;
  hipLaunchKernelGGL(slg::bool_filter_kernel, dim3((b->n_slices + per_block - 1) / per_block), dim3(slg::kBoolThreads),
                     0, st, p);
  SLG_HIP(hipGetLastError());
}
