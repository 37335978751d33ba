// slg_phrase.hip — phrase batches (slg_batch_prepare_phrase): the planned phrase tables onto the device and the
// launch of phrase_filter_kernel between the batch's scoring kernel and its select, where a bool batch launches
// bool_filter_kernel.  (The checks of a spec and the tables themselves: slg_plan.cpp, check_phrase / plan_phrase;
// the term groups' tables go up through bool_attach; the positions: slg_index.hip, slg_index_set_positions.)
#include "slg_host.hpp"

#include "slg_phrase.hpp"

using namespace slghost;

static_assert(sizeof(slg::PhraseQuery) == 32 && sizeof(slg::PhraseVar) == 16 && sizeof(slg::PhraseTerm) == 24 &&
                  sizeof(slg::PosSegDev) == 16,
              "the tables are read in whole words, the terms 8-byte aligned behind the records before them");

void slghost::phrase_attach(slg_batch *b, const slgplan::PhrasePlan &pp) {
  b->phrase = true;
  b->phrase_vars = (uint32_t)pp.vars.size();
  b->phrase_terms = (uint32_t)pp.terms.size();
  upload_image(b->d_phrase_desc, &b->idx->pool, {image_part(pp.queries), image_part(pp.vars), image_part(pp.terms)});
}

void slghost::phrase_launch(slg_batch *b, hipStream_t st) {
  if (b->n_slices == 0 || b->bool_groups == 0) return;  // nothing was scored, or no query has a clause table
  if (!b->cand_mode) throw SlgError(SLG_ERR_INTERNAL, "a phrase batch was not planned in candidates mode");
  slg::PhraseFilterParams p{};
  fill_clause_filter(p.b, b);
  p.pos_segs = b->snap->d_pos_segs.as<slg::PosSegDev>();
  unsigned char *const pd = b->d_phrase_desc.as<unsigned char>();
  p.pqueries = reinterpret_cast<const slg::PhraseQuery *>(pd);
  p.vars = reinterpret_cast<const slg::PhraseVar *>(pd + (size_t)b->nq * sizeof(slg::PhraseQuery));
  p.pterms = reinterpret_cast<const slg::PhraseTerm *>(pd + (size_t)b->nq * sizeof(slg::PhraseQuery) +
                                                       (size_t)b->phrase_vars * sizeof(slg::PhraseVar));
  constexpr uint32_t per_block = slg::kPhraseThreads / 64;
  hipLaunchKernelGGL(slg::phrase_filter_kernel, dim3((b->n_slices + per_block - 1) / per_block),
                     dim3(slg::kPhraseThreads), 0, st, p);
  SLG_HIP(hipGetLastError());
}
