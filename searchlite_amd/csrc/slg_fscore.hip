// slg_fscore.hip — function_score batches (slg_batch_prepare_fscore): the planned tables onto the device and the
// launch of fscore_kernel between the batch's scoring kernel and its select.  (The checks of a spec and the tables
// themselves: slg_plan.cpp, check_fscore / plan_fscore.)
#include "slg_host.hpp"

#include "slg_fscore.hpp"

using namespace slghost;

static_assert(sizeof(slg::FscoreQuery) == 32 && sizeof(slg::FscoreFn) == 64 && sizeof(slg::ColumnDev) == 16,
              "the tables are read in whole words, functions and columns 8-byte aligned");
static_assert(slg::kFsWeight == SLG_FSCORE_WEIGHT && slg::kFsFieldValue == SLG_FSCORE_FIELD_VALUE_FACTOR &&
                  slg::kFsDecay == SLG_FSCORE_DECAY, "header kinds");
static_assert(slg::kFsModNone == SLG_FSCORE_MOD_NONE && slg::kFsModLog == SLG_FSCORE_MOD_LOG &&
                  slg::kFsModLog1p == SLG_FSCORE_MOD_LOG1P && slg::kFsModLog2p == SLG_FSCORE_MOD_LOG2P &&
                  slg::kFsModSqrt == SLG_FSCORE_MOD_SQRT && slg::kFsModReciprocal == SLG_FSCORE_MOD_RECIPROCAL,
              "header modifiers");
static_assert(slg::kFsDecayExp == SLG_FSCORE_DECAY_EXP && slg::kFsDecayGauss == SLG_FSCORE_DECAY_GAUSS &&
                  slg::kFsDecayLinear == SLG_FSCORE_DECAY_LINEAR, "header decay functions");
static_assert(slg::kFsSum == SLG_FSCORE_MODE_SUM && slg::kFsMultiply == SLG_FSCORE_MODE_MULTIPLY &&
                  slg::kFsMax == SLG_FSCORE_MODE_MAX && slg::kFsMin == SLG_FSCORE_MODE_MIN &&
                  slg::kFsAvg == SLG_FSCORE_MODE_AVG, "header score modes");
static_assert(slg::kFsBoostMultiply == SLG_FSCORE_BOOST_MULTIPLY && slg::kFsBoostSum == SLG_FSCORE_BOOST_SUM &&
                  slg::kFsBoostReplace == SLG_FSCORE_BOOST_REPLACE && slg::kFsBoostMax == SLG_FSCORE_BOOST_MAX &&
                  slg::kFsBoostMin == SLG_FSCORE_BOOST_MIN, "header boost modes");
static_assert(slg::kFsHasMaxBoost == SLG_FSCORE_HAS_MAX_BOOST && slg::kFsHasMinScore == SLG_FSCORE_HAS_MIN_SCORE,
              "header flags");

// the fields of the batch's index state as the planner sees them
std::vector<slgplan::FscoreFieldView> slghost::fscore_field_views(const IndexState &S) {
  std::vector<slgplan::FscoreFieldView> views;
  views.reserve(S.agg_fields.size());
  for (const auto &kv : S.agg_fields) {
    slgplan::FscoreFieldView v;
    v.id = kv.first;
    v.keyword = kv.second->kind == 2;
    v.non_finite = kv.second->non_finite;
    v.n_ords = kv.second->n_ords;
    v.from_i64 = kv.second->from_i64;
    v.i64_rounded = kv.second->i64_rounded;
    v.any_value = kv.second->any_value;
    v.vmin = kv.second->vmin;
    v.vmax = kv.second->vmax;
    v.per_seg.assign(S.segs.size(), slg::ColumnDev{nullptr, nullptr});
    for (size_t s = 0; s < S.segs.size() && s < kv.second->per_seg.size(); s++)
      if (const auto &c = kv.second->per_seg[s])
        v.per_seg[s] = slg::ColumnDev{c->offs.as<const uint32_t>(), c->vals.p};
    views.push_back(std::move(v));
  }
  return views;
}

void slghost::fscore_attach(slg_batch *b, const slgplan::FscorePlan &fp) {
  b->fscore = true;
  b->fscore_work = fp.n_work;
  b->fscore_full = fp.full;
  b->fscore_fns = (uint32_t)fp.fns.size();
  b->fscore_cols = (uint32_t)fp.cols.size();
  upload_image(b->d_fscore_desc, &b->idx->pool,
               {image_part(fp.queries), image_part(fp.fns), image_part(fp.cols), image_part(fp.filters)});
}

void slghost::fscore_launch(slg_batch *b, hipStream_t st) {
  if (b->n_slices == 0 || b->fscore_work == 0) return;  // nothing was scored, or no query has work
  if (!b->cand_mode) throw SlgError(SLG_ERR_INTERNAL, "a function_score batch was not planned in candidates mode");
  slg::FscoreParams p{};
  p.c.segs = b->snap->d_segs.as<slg::SegDev>();
  p.c.sq = b->d_sq;
  p.c.slice_sq = b->d_slice_sq;
  p.c.cand = b->d_cand.as<uint2>();
  p.c.slice_cbeg = b->d_slice_cbeg.as<uint64_t>();
  p.c.slice_ccnt = b->d_slice_ccnt.as<uint32_t>();
  p.c.q_scored = b->d_q_scored.as<uint32_t>();
  p.c.n_slices = b->n_slices;
  p.c.n_segs = (uint32_t)b->snap->segs.size();
  unsigned char *base = b->d_fscore_desc.as<unsigned char>();
  p.queries = reinterpret_cast<const slg::FscoreQuery *>(base);
  base += (size_t)b->nq * sizeof(slg::FscoreQuery);
  p.fns = reinterpret_cast<const slg::FscoreFn *>(base);
  base += (size_t)b->fscore_fns * sizeof(slg::FscoreFn);
  p.cols = reinterpret_cast<const slg::ColumnDev *>(base);
  base += (size_t)b->fscore_cols * sizeof(slg::ColumnDev);
  p.filters = reinterpret_cast<const uint32_t *const *>(base);
  constexpr uint32_t per_block = slg::kFscoreThreads / 64;
  const dim3 grid((b->n_slices + per_block - 1) / per_block), block(slg::kFscoreThreads);
  if (b->fscore_full) hipLaunchKernelGGL(slg::fscore_kernel<true>, grid, block, 0, st, p);
  else hipLaunchKernelGGL(slg::fscore_kernel<false>, grid, block, 0, st, p);
  SLG_HIP(hipGetLastError());
}

extern "C" int slg_batch_fscore_info(const slg_batch *b, uint32_t *out_variant, uint32_t *out_queries_with_work) {
  return guarded([&] {
    SLG_REQUIRE(b != nullptr, "batch is NULL");
    SLG_REQUIRE(b->fscore, "not a function_score batch (slg_batch_prepare_fscore)");
    if (out_variant) *out_variant = (b->n_slices == 0 || b->fscore_work == 0) ? 0u : (b->fscore_full ? 2u : 1u);
    if (out_queries_with_work) *out_queries_with_work = b->fscore_work;
  });
}
