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
  slg_index *ix = b->idx;
  b->phrase = true;
  b->phrase_vars = (uint32_t)pp.vars.size();
  b->phrase_terms = (uint32_t)pp.terms.size();
  const size_t q_bytes = pp.queries.size() * sizeof(slg::PhraseQuery), v_bytes = pp.vars.size() * sizeof(slg::PhraseVar),
               t_bytes = pp.terms.size() * sizeof(slg::PhraseTerm);
  std::vector<unsigned char> image(q_bytes + v_bytes + t_bytes);
  if (q_bytes) std::memcpy(image.data(), pp.queries.data(), q_bytes);
  if (v_bytes) std::memcpy(image.data() + q_bytes, pp.vars.data(), v_bytes);
  if (t_bytes) std::memcpy(image.data() + q_bytes + v_bytes, pp.terms.data(), t_bytes);
  b->d_phrase_desc.alloc_pooled(&ix->pool, image.size());
  if (!image.empty()) SLG_HIP(hipMemcpy(b->d_phrase_desc.p, image.data(), image.size(), hipMemcpyHostToDevice));
}

void slghost::phrase_launch(slg_batch *b, hipStream_t st) {
  if (b->n_slices == 0 || b->bool_groups == 0) return;  // nothing was scored, or no query has a clause table
  if (!b->cand_mode) throw SlgError(SLG_ERR_INTERNAL, "a phrase batch was not planned in candidates mode");
  const IndexState &S = *b->snap;
  slg::PhraseFilterParams p{};
  p.segs = S.d_segs.as<slg::SegDev>();
  p.pos_segs = S.d_pos_segs.as<slg::PosSegDev>();
  p.sq = b->d_sq;
  p.slice_sq = b->d_slice_sq;
  p.queries = b->d_bool_desc.as<const slg::BoolQuery>();
  p.terms = reinterpret_cast<const slg::BoolTerm *>(b->d_bool_desc.as<unsigned char>() +
                                                    (size_t)b->nq * sizeof(slg::BoolQuery));
  unsigned char *const pd = b->d_phrase_desc.as<unsigned char>();
  p.pqueries = reinterpret_cast<const slg::PhraseQuery *>(pd);
  p.vars = reinterpret_cast<const slg::PhraseVar *>(pd + (size_t)b->nq * sizeof(slg::PhraseQuery));
  p.pterms = reinterpret_cast<const slg::PhraseTerm *>(pd + (size_t)b->nq * sizeof(slg::PhraseQuery) +
                                                       (size_t)b->phrase_vars * sizeof(slg::PhraseVar));
  p.cand = b->d_cand.as<uint2>();
  p.slice_cbeg = b->d_slice_cbeg.as<uint64_t>();
  p.slice_ccnt = b->d_slice_ccnt.as<uint32_t>();
  p.q_scored = b->d_q_scored.as<uint32_t>();
  p.n_slices = b->n_slices;
  p.n_segs = (uint32_t)S.segs.size();
  constexpr uint32_t per_block = slg::kPhraseThreads / 64;
  hipLaunchKernelGGL(slg::phrase_filter_kernel, dim3((b->n_slices + per_block - 1) / per_block),
                     dim3(slg::kPhraseThreads), 0, st, p);
  SLG_HIP(hipGetLastError());
}
