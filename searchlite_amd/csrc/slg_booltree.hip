// slg_booltree.hip — tree batches (slg_batch_prepare_bool_tree): the planned matcher tables onto the device and the
// launch of booltree_filter_kernel between the batch's scoring kernel and its select.  (The checks of a spec and
// the tables themselves: slg_plan.cpp, check_bool_tree / plan_bool_tree.)
#include "slg_host.hpp"

#include "slg_booltree.hpp"

using namespace slghost;

static_assert(sizeof(slg::BoolTreeQuery) == 32 && sizeof(slg::BoolTreeNode) == 32 && sizeof(slg::BoolTerm) == 16,
              "the tables are read in whole words; nodes, terms and addresses 8-byte aligned behind the records");

void slghost::booltree_attach(slg_batch *b, const slgplan::BoolTreePlan &tp) {
  b->booltree = true;
  b->bt_nodes = (uint32_t)tp.nodes.size();
  b->bt_terms = (uint32_t)tp.terms.size();
  b->bt_filters = (uint32_t)tp.filters.size();
  upload_image(b->d_booltree_desc, &b->idx->pool,
               {image_part(tp.queries), image_part(tp.nodes), image_part(tp.terms), image_part(tp.filters),
                image_part(tp.filt_rows)});
}

void slghost::booltree_launch(slg_batch *b, hipStream_t st) {
  if (b->n_slices == 0 || b->bt_nodes == 0) return;  // nothing was scored, or no query has a matcher
  if (!b->cand_mode) throw SlgError(SLG_ERR_INTERNAL, "a tree batch was not planned in candidates mode");
  slg::BoolTreeParams p{};
  p.c.segs = b->snap->d_segs.as<slg::SegDev>();
  p.c.sq = b->d_sq;
  p.c.slice_sq = b->d_slice_sq;
  p.c.cand = b->d_cand.as<uint2>();
  p.c.slice_cbeg = b->d_slice_cbeg.as<uint64_t>();
  p.c.slice_ccnt = b->d_slice_ccnt.as<uint32_t>();
  p.c.q_scored = b->d_q_scored.as<uint32_t>();
  p.c.n_slices = b->n_slices;
  p.c.n_segs = (uint32_t)b->snap->segs.size();
  unsigned char *base = b->d_booltree_desc.as<unsigned char>();
  p.queries = reinterpret_cast<const slg::BoolTreeQuery *>(base);
  base += (size_t)b->nq * sizeof(slg::BoolTreeQuery);
  p.nodes = reinterpret_cast<const slg::BoolTreeNode *>(base);
  base += (size_t)b->bt_nodes * sizeof(slg::BoolTreeNode);
  p.c.terms = reinterpret_cast<const slg::BoolTerm *>(base);
  base += (size_t)b->bt_terms * sizeof(slg::BoolTerm);
  p.filters = reinterpret_cast<const uint32_t *const *>(base);
  base += (size_t)b->bt_filters * sizeof(void *);
  p.filt_rows = reinterpret_cast<const uint32_t *>(base);
  constexpr uint32_t per_block = slg::kBoolTreeThreads / 64;
  hipLaunchKernelGGL(slg::booltree_filter_kernel, dim3((b->n_slices + per_block - 1) / per_block),
                     dim3(slg::kBoolTreeThreads), 0, st, p);
  SLG_HIP(hipGetLastError());
}
