// slg_script.hip — script_score batches (slg_batch_prepare_script): the planned tables onto the device and the
// launch of script_kernel between the batch's scoring kernel and its select, alone or beside the function_score
// stage.  (The checks of a spec and the tables themselves: slg_plan.cpp, check_script / plan_script.)
#include "slg_host.hpp"

#include "slg_script.hpp"

using namespace slghost;

static_assert(sizeof(slg::ScriptQuery) == 64 && sizeof(slg::ScriptInstr) == 16 && sizeof(slg::ColumnDev) == 16,
              "the tables are read in whole words, instructions and columns 8-byte aligned");
static_assert(slg::kScPushConst == SLG_SCRIPT_PUSH_CONST && slg::kScPushField == SLG_SCRIPT_PUSH_FIELD &&
                  slg::kScPushScore == SLG_SCRIPT_PUSH_SCORE && slg::kScAdd == SLG_SCRIPT_ADD &&
                  slg::kScSub == SLG_SCRIPT_SUB && slg::kScMul == SLG_SCRIPT_MUL && slg::kScDiv == SLG_SCRIPT_DIV &&
                  slg::kScNeg == SLG_SCRIPT_NEG, "header ops");
static_assert(slg::kScriptMaxDepth == 8 && slg::kScriptMaxFields == 8, "the kernel's eight slots and eight field values");

void slghost::script_attach(slg_batch *b, const slgplan::ScriptPlan &sp, bool first) {
  b->script = true;
  b->script_first = first;
  b->script_work = sp.n_work;
  b->script_max_depth = sp.max_depth;
  b->script_instrs = (uint32_t)sp.instrs.size();
  upload_image(b->d_script_desc, &b->idx->pool, {image_part(sp.queries), image_part(sp.instrs), image_part(sp.cols)});
}

void slghost::script_launch(slg_batch *b, hipStream_t st) {
  if (b->n_slices == 0 || b->script_work == 0) return;  // nothing was scored, or no query has a program
  if (!b->cand_mode) throw SlgError(SLG_ERR_INTERNAL, "a script_score batch was not planned in candidates mode");
  slg::ScriptParams p{};
  p.c.segs = b->snap->d_segs.as<slg::SegDev>();
  p.c.sq = b->d_sq;
  p.c.slice_sq = b->d_slice_sq;
  p.c.cand = b->d_cand.as<uint2>();
  p.c.slice_cbeg = b->d_slice_cbeg.as<uint64_t>();
  p.c.slice_ccnt = b->d_slice_ccnt.as<uint32_t>();
  p.c.q_scored = b->d_q_scored.as<uint32_t>();
  p.c.n_slices = b->n_slices;
  p.c.n_segs = (uint32_t)b->snap->segs.size();
  unsigned char *base = b->d_script_desc.as<unsigned char>();
  p.queries = reinterpret_cast<const slg::ScriptQuery *>(base);
  base += (size_t)b->nq * sizeof(slg::ScriptQuery);
  p.instrs = reinterpret_cast<const slg::ScriptInstr *>(base);
  base += (size_t)b->script_instrs * sizeof(slg::ScriptInstr);
  p.cols = reinterpret_cast<const slg::ColumnDev *>(base);
  constexpr uint32_t per_block = slg::kScriptThreads / 64;
  const dim3 grid((b->n_slices + per_block - 1) / per_block), block(slg::kScriptThreads);
  hipLaunchKernelGGL(slg::script_kernel, grid, block, 0, st, p);
  SLG_HIP(hipGetLastError());
}

extern "C" int slg_batch_script_info(const slg_batch *b, uint32_t *out_queries_with_work, uint32_t *out_max_depth) {
  return guarded([&] {
    SLG_REQUIRE(b != nullptr, "batch is NULL");
    SLG_REQUIRE(b->script, "not a script_score batch (slg_batch_prepare_script)");
    if (out_queries_with_work) *out_queries_with_work = b->script_work;
    if (out_max_depth) *out_max_depth = b->script_work == 0 ? 0u : b->script_max_depth;
  });
}
