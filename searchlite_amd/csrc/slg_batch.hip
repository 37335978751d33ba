// slg_batch.hip — query batches: planning a batch onto the device (slg_batch_prepare*), the launches of one
// run, waiting, fetching and destroying, the one-call searches, and the merge of shard results.
#include "slg_host.hpp"

#include <thread>

#include "slg_kernels.hpp"
#include "slg_score.hpp"

using namespace slghost;

namespace slg {
// defined in slg_score_inst.hip, one translation unit per KREGS
template <int KREGS>
void launch_score_kregs(const RoundScoreParams &sp, int kind, hipStream_t st);
template <> void launch_score_kregs<1>(const RoundScoreParams &, int, hipStream_t);
template <> void launch_score_kregs<2>(const RoundScoreParams &, int, hipStream_t);
template <> void launch_score_kregs<4>(const RoundScoreParams &, int, hipStream_t);
template <> void launch_score_kregs<8>(const RoundScoreParams &, int, hipStream_t);
template <> void launch_score_kregs<16>(const RoundScoreParams &, int, hipStream_t);
}  // namespace slg
namespace {

// kind: 2 many-term kernel (slg_score_multi.hpp), 3 many-term kernel with pruning-classified lists,
// 6 / 7 the few-term kernel (slg_score_uni4.hpp), <= 4 / 5..8 lists; 8 / 9: the same with score plans
// (flat Sum / DisMax over leaves)
int uniform_kind(uint32_t max_terms, bool plans) {
  const bool few = max_terms <= (uint32_t)slg::kUniMaxLists;
  if (plans) return few ? 8 : 9;
  return few ? 6 : 7;
}
void launch_score(const slg::RoundScoreParams &sp, int kind, hipStream_t st) {
#ifdef SLG_STAMPS  // diagnostic build: only the k <= 64 variant is compiled
  if (kregs_for(sp.k) != 1) throw SlgError(SLG_ERR_UNSUPPORTED, "stamps build supports k <= 64 only");
  slg::launch_score_kregs<1>(sp, kind, st);
  SLG_HIP(hipGetLastError());
  return;
#else
  switch (kregs_for(sp.k)) {
    case 1: slg::launch_score_kregs<1>(sp, kind, st); break;
    case 2: slg::launch_score_kregs<2>(sp, kind, st); break;
    case 4: slg::launch_score_kregs<4>(sp, kind, st); break;
    case 8: slg::launch_score_kregs<8>(sp, kind, st); break;
    default: slg::launch_score_kregs<16>(sp, kind, st); break;
  }
  SLG_HIP(hipGetLastError());
#endif
}

// What the parameters of a batch's final kernel (merge_topk_kernel or one of the selects) have in common:
// the slices of each query in, the batch's result block and the copy of the index's error word out ...
template <typename P>
void fill_final(P &p, const slg_batch *b) {
  p.queries = b->d_queries;
  p.slice_seg = b->d_slice_seg;
  p.out_doc = b->d_out_doc;
  p.out_seg = b->d_out_seg;
  p.out_score = b->d_out_score;
  p.out_count = b->d_out_count;
  p.nq = b->nq;
  p.k = b->k;
  p.error_flag = b->idx->d_error_flag.as<uint32_t>();
  p.out_flag = ResultBlock(b->nq, b->k).flag(b->d_out.as<uint32_t>());
}
// ... and what the two selects share beyond that: the candidate regions (fill_candidates), and the matched
// counts, cursor keys and seen flags of the batches that have them (null otherwise)
template <typename P>
void fill_select(P &p, const slg_batch *b) {
  fill_final(p, b);
  fill_candidates(p, b);
  p.out_matched = b->d_matched.as<unsigned long long>();
  p.cursor = b->d_cursor.as<const uint32_t>();
  p.out_seen = b->d_seen.as<uint32_t>();
}

template <int KREGS>
void launch_merge_t(const slg::MergeParams &mp, hipStream_t st) {
  const uint32_t blocks = (mp.nq + slg::kWavesPerBlock - 1) / slg::kWavesPerBlock;
  hipLaunchKernelGGL((slg::merge_topk_kernel<KREGS>), dim3(blocks), dim3(256), 0, st, mp);
}
void launch_merge(const slg::MergeParams &mp, hipStream_t st) {
  switch (kregs_for(mp.k)) {
    case 1: launch_merge_t<1>(mp, st); break;
    case 2: launch_merge_t<2>(mp, st); break;
    case 4: launch_merge_t<4>(mp, st); break;
    case 8: launch_merge_t<8>(mp, st); break;
    default: launch_merge_t<16>(mp, st); break;
  }
  SLG_HIP(hipGetLastError());
}

template <int KREGS>
void launch_shard_merge_t(const slg::ShardMergeParams &mp, hipStream_t st) {
  const uint32_t blocks = (mp.nq + slg::kWavesPerBlock - 1) / slg::kWavesPerBlock;
  hipLaunchKernelGGL((slg::merge_shards_kernel<KREGS>), dim3(blocks), dim3(256), 0, st, mp);
}
}  // namespace

void slghost::launch_shard_merge(const slg::ShardMergeParams &mp, hipStream_t st) {
  if (mp.k > 1024u) {  // beyond the register top-k: rank every entry by binary searches
    hipLaunchKernelGGL(slg::merge_shards_large_kernel, dim3(mp.nq), dim3(256), 0, st, mp);
    SLG_HIP(hipGetLastError());
    return;
  }
  switch (kregs_for(mp.k)) {
    case 1: launch_shard_merge_t<1>(mp, st); break;
    case 2: launch_shard_merge_t<2>(mp, st); break;
    case 4: launch_shard_merge_t<4>(mp, st); break;
    case 8: launch_shard_merge_t<8>(mp, st); break;
    default: launch_shard_merge_t<16>(mp, st); break;
  }
  SLG_HIP(hipGetLastError());
}

// every part names `_score` or a field with a column for every segment (a field registered before
// slg_index_add_segment has none for the new one)
SortBinding slghost::bind_sort(const IndexState &S, const slg_sort_spec &spec, const std::string &prefix,
                               const std::string &part) {
  const size_t n_segs = S.segs.size();
  SortBinding sb;
  sb.cols.assign(slg::kSortMaxParts * std::max<size_t>(n_segs, 1), slg::SortColDev{nullptr, nullptr});
  for (uint32_t i = 0; i < spec.n_parts; i++) {
    if (spec.order[i] == SLG_ORDER_DESC) sb.desc_parts |= 1u << i;
    if (spec.field[i] == SLG_SORT_SCORE) {
      sb.score_parts |= 1u << i;
      continue;
    }
    const auto it = S.sort_fields.find(spec.field[i]);
    SLG_REQUIRE(it != S.sort_fields.end(), prefix + "unknown sort field id in " + part + std::to_string(i));
    const SortFieldData &fd = *it->second;
    for (size_t s = 0; s < n_segs; s++) {
      SLG_REQUIRE(s < fd.per_seg.size() && fd.per_seg[s],
                  prefix + "sort field " + std::to_string(spec.field[i]) + " has no column for segment " +
                      std::to_string(s) + " (added after the field was registered)");
      const SortColumn &c = *fd.per_seg[s];
      sb.cols[i * n_segs + s] = slg::SortColDev{c.key[spec.order[i]].as<const unsigned long long>(),
                                                c.present.as<const uint32_t>()};
    }
  }
  return sb;
}

void slghost::release_batch_buffers(slg_batch *b) {
  static_cast<slg_batch_buffers &>(*b) = slg_batch_buffers{};  // (each DevBuf's move assignment releases its block)
  for (hipEvent_t &e : b->ev_shard) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
}

void slghost::attach_select_buffers(slg_batch *b, const std::vector<uint32_t> &q_filter, const slg_sort_spec *sort,
                                    const SortBinding &sorting, bool counts_matched) {
  BufPool *const pool = &b->idx->pool;
  const uint32_t nq = b->nq;
  if (!q_filter.empty()) {
    b->d_q_filter.alloc_pooled(pool, (size_t)nq * 4);
    SLG_HIP(hipMemcpy(b->d_q_filter.p, q_filter.data(), (size_t)nq * 4, hipMemcpyHostToDevice));
  }
  b->sorted = sort != nullptr;
  if (b->sorted) {
    b->n_sort_parts = sort->n_parts;
    b->sort_score_parts = sorting.score_parts;
    b->sort_desc_parts = sorting.desc_parts;
    b->d_sort_cols.alloc_pooled(pool, sorting.cols.size() * sizeof(slg::SortColDev));
    SLG_HIP(hipMemcpy(b->d_sort_cols.p, sorting.cols.data(), sorting.cols.size() * sizeof(slg::SortColDev),
                      hipMemcpyHostToDevice));
  }
  if (counts_matched) b->d_matched.alloc_pooled(pool, (size_t)std::max<uint32_t>(nq, 1) * 8);
  const ResultBlock R(nq, b->k);
  b->d_out.alloc_pooled(pool, R.words_with_flag() * 4);
  b->d_out_doc = R.doc(b->d_out.as<uint32_t>());
  b->d_out_seg = R.seg(b->d_out.as<uint32_t>());
  b->d_out_score = R.score(b->d_out.as<uint32_t>());
  b->d_out_count = R.count(b->d_out.as<uint32_t>());
}

extern "C" {

slg_batch *slg_batch_prepare(slg_index *ix, uint32_t nq, const uint32_t *q_offsets,
                             const uint32_t *q_term_ids, const float *q_weights, uint32_t k,
                             int strategy) {
  return slg_batch_prepare_filtered(ix, nq, q_offsets, q_term_ids, q_weights, nullptr, k, strategy);
}

slg_batch *slg_batch_prepare_filtered(slg_index *ix, uint32_t nq, const uint32_t *q_offsets,
                                      const uint32_t *q_term_ids, const float *q_weights,
                                      const int32_t *q_filter, uint32_t k, int strategy) {
  return slg_batch_prepare_plan(ix, nq, q_offsets, q_term_ids, q_weights, nullptr, nullptr, nullptr,
                                nullptr, q_filter, k, strategy);
}

slg_batch *slg_batch_prepare_plan(slg_index *ix, uint32_t nq, const uint32_t *q_offsets,
                                  const uint32_t *q_term_ids, const float *q_weights,
                                  const uint32_t *q_leaf, const int32_t *q_plan, const float *q_tie,
                                  const uint32_t *q_nleaves, const int32_t *q_filter, uint32_t k,
                                  int strategy) {
  slg_score_plans pl{};
  pl.q_leaf = q_leaf;
  pl.q_plan = q_plan;
  pl.q_tie = q_tie;
  pl.q_nleaves = q_nleaves;
  return slg_batch_prepare_plans(ix, nq, q_offsets, q_term_ids, q_weights, &pl, q_filter, k, strategy);
}

}  // extern "C"

// The kinds one batch may hold together (searchlite_gpu.h, "compound requests").  Only
// slg_batch_prepare_request can ask for a pair this refuses: each legacy entry sets one legal combination.
// Needs no index; the message names the pair.
static void check_request(const PrepareRequest &r) {
  auto refuse = [](const char *a, const char *b, const char *why) {
    throw SlgError(SLG_ERR_UNSUPPORTED, std::string(a) + " with " + b + ": " + why);
  };
  // (a phrase batch's bool spec is its own term groups: boolean.on beside phrase.on is one clause kind)
  const char *const clause = r.phrase.on ? "phrase_spec" : r.boolean.on ? "bool_spec" : nullptr;
  if (r.booltree.on && clause) refuse("bool_tree_spec", clause, "one clause stage per request");
  struct Named {
    bool on;
    const char *name;
  };
  const Named family[3] = {{r.top_hits.on, "top_hits"}, {r.composite.on, "composite"}, {r.term_buckets.on, "term_buckets"}};
  const Named collectors[4] = {{r.aggs.on, "aggs"}, family[0], family[1], family[2]};
  for (int i = 0; i < 3; i++)
    for (int j = i + 1; j < 3; j++)
      if (family[i].on && family[j].on) refuse(family[i].name, family[j].name, "one of the three beside aggs");
  if (r.cursor.on)
    for (const Named &c : collectors)
      if (c.on) refuse("q_cursor", c.name, "the collectors do not test the cursor");
  if (r.rescore.on) {
    const Named others[] = {{r.sort.on, "sort"},   {r.cursor.on, "q_cursor"}, {r.fscore.on, "fscore_spec"},
                            {r.script.on, "script_spec"}, collectors[0], collectors[1], collectors[2], collectors[3],
                            {r.collapse.on, "collapse"}};
    for (const Named &o : others)
      if (o.on) refuse("rescore", o.name, "rescore runs in score order behind at most a clause stage");
  }
}

// every slg_batch_prepare*: the kinds the request asks for decide what is checked, planned and attached
slg_batch *slghost::prepare_impl(const PrepareRequest &r) {
  slg_index *const ix = r.ix;
  const uint32_t nq = r.nq, k = r.k;
  const slg_score_plans *const plans = r.plans;
  const slg_sort_spec *const sort = r.sort.spec;
  const slg_sort_cursor *const q_cursor = r.cursor.spec;
  const bool after = r.cursor.on, hybrid = r.hybrid;
  return prepare_guarded([&](slg_batch *&b) {
    SLG_REQUIRE(!r.sort.on || sort != nullptr, "sort spec is NULL");
    if (r.aggs.on) agg_check_spec(r.aggs.spec);  // (what needs no index comes first, as every argument check)
    if (r.rescore.on) slgplan::check_rescore(r.rescore.spec, nq, k);
    if (r.phrase.on) slgplan::check_phrase(r.boolean.spec, r.phrase.spec, nq, plans);
    else if (r.boolean.on) slgplan::check_bool(r.boolean.spec, nq, plans);
    if (r.booltree.on) slgplan::check_bool_tree(r.booltree.spec, nq, plans);
    if (r.fscore.on) slgplan::check_fscore(r.fscore.spec, nq);
    slgplan::ScriptShape script_shape;
    if (r.script.on) {
      slgplan::check_script_order(r.script_order);  // (an invalid argument comes before an unsupported program)
      slgplan::check_script(r.script.spec, nq, script_shape);
    }
    if (r.collapse.on) slgplan::check_collapse(r.collapse.spec, k);
    if (r.top_hits.on) slgplan::check_top_hits(r.top_hits.spec, r.aggs.spec);
    if (r.composite.on) composite_check_spec(r.composite.spec);
    if (r.term_buckets.on) term_buckets_check_spec(r.term_buckets.spec);
    check_request(r);  // (behind every kind's own checks: an invalid argument comes before an unsupported pair)
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(!after || q_cursor != nullptr, "q_cursor is NULL");
    check_sort_spec(sort);  // (before planning: the planner never sees a sort spec it cannot run)
    // Planning (slg_plan.cpp: a pure host function) reads only the immutable state the batch binds
    // to, so host threads may prepare batches for one index concurrently, also while an update builds
    // the next state; the index mutex is held just to take the snapshot.
    const std::shared_ptr<const IndexState> snap = ix->snapshot();
    const std::vector<char> filter_live = filter_liveness(*snap);
    std::vector<slgplan::SegView> views(snap->segs.size());
    for (size_t s = 0; s < snap->segs.size(); s++) {
      const SegHost &sh = *snap->segs[s];
      views[s].n_docs = sh.n_docs;
      views[s].n_terms = sh.n_terms;
      views[s].term_offsets = sh.store->term_offsets.data();
      views[s].champ = sh.champ.empty() ? nullptr : sh.champ.data();
      views[s].has_positions = s < snap->positions.size() && snap->positions[s] != nullptr;
    }
    slgplan::BatchIn in;
    in.nq = nq;
    in.q_offsets = r.q_offsets;
    in.q_term_ids = r.q_term_ids;
    in.q_weights = r.q_weights;
    if (plans) in.plans = *plans;
    in.q_filter = r.q_filter;
    in.k = k;
    in.strategy = r.strategy;
    in.filter_live = filter_live.data();
    in.n_filters = filter_live.size();
    in.sorted = r.plans_every_match();
    SortBinding sorting;  // the columns of the sort parts in the batch's state
    if (sort) sorting = bind_sort(*snap, *sort, "", "part ");
    // the cursors as the key words the select kernel compares (against the same snapshot's field kinds)
    std::vector<uint32_t> cursor_words;
    if (after) {
      int kind[SLG_MAX_SORT_PARTS] = {0, 0, 0, 0};
      const uint32_t n_parts = sort ? sort->n_parts : 0u;
      for (uint32_t i = 0; i < n_parts; i++)
        kind[i] = sort->field[i] == SLG_SORT_SCORE ? 0 : snap->sort_fields.at(sort->field[i])->kind;
      cursor_words.assign((size_t)std::max<uint32_t>(nq, 1) * slg::kCursorStride, 0u);
      for (uint32_t q = 0; q < nq; q++) {
        if (!q_cursor[q].has_cursor) continue;
        uint32_t *w = &cursor_words[(size_t)q * slg::kCursorStride];
        w[0] = 1u;
        try {
          slgplan::cursor_key(n_parts, kind, sort ? sort->order : nullptr, q_cursor[q], w + 1);
        } catch (const slgplan::SlgError &e) {
          throw SlgError(e.code, "query " + std::to_string(q) + ": " + e.what());
        }
      }
    }
    slgplan::Plan plan;
    slgplan::plan_batch(views, ix->tune, in, plan);
    slgplan::RescorePlan rescore_plan;  // (against the same snapshot, before any device work)
    if (r.rescore.on) slgplan::plan_rescore(views, nq, k, *r.rescore.spec, rescore_plan);
    slgplan::BoolPlan bool_plan;
    slgplan::PhrasePlan phrase_plan;
    if (r.phrase.on) slgplan::plan_phrase(views, nq, r.boolean.spec, *r.phrase.spec, phrase_plan);
    else if (r.boolean.on) slgplan::plan_bool(views, nq, *r.boolean.spec, bool_plan);
    slgplan::BoolTreePlan booltree_plan;
    if (r.booltree.on)
      slgplan::plan_bool_tree(views, snap->reject_host.data(), filter_live.data(), filter_live.size(), nq,
                              *r.booltree.spec, booltree_plan);
    slgplan::FscorePlan fscore_plan;
    if (r.fscore.on)
      slgplan::plan_fscore(fscore_field_views(*snap), snap->reject_host.data(), filter_live.data(), filter_live.size(),
                           (uint32_t)snap->segs.size(), nq, *r.fscore.spec, fscore_plan);
    slgplan::ScriptPlan script_plan;
    if (r.script.on)
      slgplan::plan_script(fscore_field_views(*snap), (uint32_t)snap->segs.size(), nq, *r.script.spec, script_shape,
                           script_plan);

    DeviceGuard g(ix->device);
    b = new slg_batch();
    b->idx = ix;
    b->snap = snap;
    b->nq = nq;
    b->k = k;
    b->strategy = r.strategy;
    b->q_postings.swap(plan.q_postings);
    b->n_postings = plan.n_postings;
    b->n_postings_essential = plan.n_postings_essential;
    b->n_postings_nonessential = plan.n_postings_nonessential;
    b->n_rounds = plan.n_rounds;
    b->max_terms = plan.max_terms;
    b->uniform = plan.uniform;
    b->multi = plan.multi;
    b->plan_batch = plan.plan_batch;
    b->nested = plan.nested;
    b->deep = plan.deep;
    b->pruned = plan.pruned;
    b->cand_mode = plan.cand_mode;
    b->after = after;
    b->hybrid = hybrid;
    b->score_k = slgplan::planning_k(in);
    b->n_sq = (uint32_t)plan.sqs.size();
    b->n_terms = (uint32_t)plan.terms.size();
    b->n_slices = (uint32_t)plan.slice_sq.size();
    b->n_boundaries = (uint32_t)plan.n_bnd;
    {  // what slg_batch_explain looks a row's lists up with: the sub-query of every (query, segment) pair
      const size_t n_segs = snap->segs.size();
      b->ex_q_seg_sq.assign((size_t)nq * n_segs, 0xFFFFFFFFu);
      std::vector<uint32_t> q_rows(nq, 0u);
      for (size_t i = 0; i < plan.sqs.size(); i++) {
        const slg::RoundQuery &sq = plan.sqs[i];
        if (sq.q >= nq || sq.seg >= n_segs) throw SlgError(SLG_ERR_INTERNAL, "a sub-query of no query or segment");
        b->ex_q_seg_sq[(size_t)sq.q * n_segs + sq.seg] = (uint32_t)i;
        q_rows[sq.q] += sq.n_terms;
        b->ex_max_table = std::max(b->ex_max_table, q_rows[sq.q]);
      }
    }

    // ---- the descriptor image: one H2D copy the caller waits for, outside any lock, on an upload
    // stream of its own.  (Measured against an image copied asynchronously on the batch's stream in
    // front of the kernels: that variant served 5.2-7.4M queries/s from 4-8 caller threads where
    // this one serves 8.0-8.8M — the stream-ordered copy delays each batch's first kernel.)  The
    // staging image is pinned, so the copy is one DMA at PCIe speed (26 MB: 0.6 ms; from pageable
    // memory 1-6 ms), and comes from the index's free list (a fresh 26 MB vector per config-4
    // batch spent half of its 5 ms in page faults); it goes back when prepare returns.
    const size_t total = plan.image_bytes;
    ImageLease lease(ix->pool, total ? total : 16);
    plan.pack(static_cast<unsigned char *>(lease.p));
    b->d_desc.alloc_pooled(&ix->pool, total);
    {
      hipStream_t us = ix->upload_streams[std::hash<std::thread::id>()(std::this_thread::get_id()) %
                                          slg_index::kUploadStreams];
      SLG_HIP(hipMemcpyAsync(b->d_desc.p, lease.p, total, hipMemcpyHostToDevice, us));
      SLG_HIP(wait_stream(us));
    }
    unsigned char *db = b->d_desc.as<unsigned char>();
    b->d_sq = reinterpret_cast<const slg::RoundQuery *>(db + plan.o_sq);
    b->d_terms = reinterpret_cast<const slg::TermRef *>(db + plan.o_terms);
    b->d_slice_sq = reinterpret_cast<const uint32_t *>(db + plan.o_slice);
    b->d_slice_seg = reinterpret_cast<const uint32_t *>(db + plan.o_sseg);
    b->d_slice_order = reinterpret_cast<const uint32_t *>(db + plan.o_sord);
    b->d_queries = reinterpret_cast<const slg::QueryRef *>(db + plan.o_q);
    b->d_bnd_coarse = reinterpret_cast<const uint32_t *>(db + plan.o_bc);
    b->d_nodes = reinterpret_cast<const slg::PlanNode *>(db + plan.o_nodes);
    b->d_bounds.alloc_pooled(&ix->pool, (size_t)plan.n_bounds * 4);
    b->d_rdoc.alloc_pooled(&ix->pool, (size_t)plan.n_bnd * 4);
    b->d_slice_desc.alloc_pooled(&ix->pool, (size_t)b->n_slices * sizeof(slg::SliceDesc));
    if (b->cand_mode) {
      b->d_cand.alloc_pooled(&ix->pool, (size_t)(plan.cand_total + 1) * 8);
      b->d_slice_cbeg.alloc_pooled(&ix->pool, (size_t)b->n_slices * 8);
      b->d_slice_ccnt.alloc_pooled(&ix->pool, (size_t)b->n_slices * 4);
    } else {
      b->d_slice_tk.alloc_pooled(&ix->pool, (size_t)b->n_slices * k * 4);
      b->d_slice_doc.alloc_pooled(&ix->pool, (size_t)b->n_slices * k * 4);
    }
    b->d_q_scored.alloc_pooled(&ix->pool, (size_t)nq * 4);
    // (from the pool like every per-batch buffer: a raw hipMalloc / hipFree per batch synchronises
    // the device and cost config 4's two-in-flight pipeline 60 %)
    if (b->pruned && !b->uniform && ix->tune.block_max) b->d_blk_skip.alloc_pooled(&ix->pool, ((size_t)nq + 1) * 8);
    attach_select_buffers(b, plan.q_filter, sort, sorting, r.counts_matched());
    if (b->after) {
      b->d_cursor.alloc_pooled(&ix->pool, cursor_words.size() * 4);
      SLG_HIP(hipMemcpy(b->d_cursor.p, cursor_words.data(), cursor_words.size() * 4, hipMemcpyHostToDevice));
      b->d_seen.alloc_pooled(&ix->pool, (size_t)std::max<uint32_t>(nq, 1) * 4);
    }
    if (b->hybrid) {  // where each query's candidates start: its sub-queries' regions lie one after another
      b->q_cand.assign((size_t)nq + 1, UINT64_MAX);
      b->q_cand[nq] = plan.cand_total;
      uint64_t prev = 0;
      for (const slg::RoundQuery &sq : plan.sqs) {
        const uint64_t base = ((uint64_t)sq.cand_hi << 32) | sq.cand_lo;
        // (hy_gather_kernel searches the slices' regions by slot: they must lie in sub-query, so query, order)
        if (base < prev || sq.q >= nq) throw SlgError(SLG_ERR_INTERNAL, "candidate regions are not in query order");
        prev = base;
        b->q_cand[sq.q] = std::min(b->q_cand[sq.q], base);
      }
      for (uint32_t q = nq; q-- > 0;)
        if (b->q_cand[q] == UINT64_MAX) b->q_cand[q] = b->q_cand[q + 1];
      b->d_q_cand.alloc_pooled(&ix->pool, b->q_cand.size() * 8);
      SLG_HIP(hipMemcpy(b->d_q_cand.p, b->q_cand.data(), b->q_cand.size() * 8, hipMemcpyHostToDevice));
    }
    if (r.aggs.on) agg_attach(b, *r.aggs.spec);
    if (r.top_hits.on) top_hits_attach(b, *r.top_hits.spec);
    if (r.composite.on) composite_attach(b, *r.composite.spec);
    if (r.term_buckets.on) term_buckets_attach(b, *r.term_buckets.spec);
    if (r.rescore.on) rescore_attach(b, rescore_plan);
    if (r.phrase.on) {
      bool_attach(b, phrase_plan.bools);
      phrase_attach(b, phrase_plan);
    } else if (r.boolean.on) {
      bool_attach(b, bool_plan);
    }
    if (r.booltree.on) booltree_attach(b, booltree_plan);
    if (r.fscore.on) fscore_attach(b, fscore_plan);
    if (r.script.on) script_attach(b, script_plan, r.fscore.on && r.script_order == SLG_SCRIPT_INNER);
    if (r.collapse.on) collapse_attach(b, *r.collapse.spec, sort);
  });
}

extern "C" {

slg_batch *slg_batch_prepare_plans(slg_index *ix, uint32_t nq, const uint32_t *q_offsets,
                                   const uint32_t *q_term_ids, const float *q_weights,
                                   const slg_score_plans *plans, const int32_t *q_filter, uint32_t k,
                                   int strategy) {
  return prepare_impl(PrepareRequest{ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy});
}

slg_batch *slg_batch_prepare_sorted(slg_index *ix, uint32_t nq, const uint32_t *q_offsets,
                                    const uint32_t *q_term_ids, const float *q_weights,
                                    const slg_score_plans *plans, const int32_t *q_filter,
                                    const slg_sort_spec *sort, uint32_t k, int strategy) {
  PrepareRequest r{ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy};
  r.sort = {true, sort};
  return prepare_impl(r);
}

slg_batch *slg_batch_prepare_after(slg_index *ix, uint32_t nq, const uint32_t *q_offsets,
                                   const uint32_t *q_term_ids, const float *q_weights,
                                   const slg_score_plans *plans, const int32_t *q_filter, const slg_sort_spec *sort,
                                   const slg_sort_cursor *q_cursor, uint32_t k, int strategy) {
  PrepareRequest r{ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy};
  r.sort = if_given(sort);
  r.cursor = {true, q_cursor};
  return prepare_impl(r);
}

// a compound request: every kind whose pointer is given, through the one path of the calls above and below
slg_batch *slg_batch_prepare_request(slg_index *ix, const slg_request *req) {
  const int rc = guarded([&] {
    SLG_REQUIRE(req != nullptr, "req is NULL");
    SLG_REQUIRE(req->struct_size == sizeof(slg_request), "slg_request.struct_size is not sizeof(slg_request)");
    SLG_REQUIRE(req->reserved == 0u, "slg_request.reserved is not 0");
  });
  if (rc != SLG_OK) return nullptr;
  PrepareRequest r{ix, req->nq, req->q_offsets, req->q_term_ids, req->q_weights, req->plans, req->q_filter, req->k,
                   req->strategy};
  r.sort = if_given(req->sort);
  r.cursor = if_given(req->q_cursor);
  r.phrase = if_given(req->phrase_spec);
  r.boolean = {req->bool_spec != nullptr || req->phrase_spec != nullptr, req->bool_spec};  // (as slg_batch_prepare_phrase)
  r.booltree = if_given(req->bool_tree_spec);
  r.fscore = if_given(req->fscore_spec);
  r.script = if_given(req->script_spec);
  r.script_order = req->script_spec ? req->script_order : SLG_SCRIPT_OUTER;
  r.aggs = if_given(req->aggs);
  r.top_hits = if_given(req->top_hits);
  r.composite = if_given(req->composite);
  r.term_buckets = if_given(req->term_buckets);
  r.rescore = if_given(req->rescore);
  r.collapse = if_given(req->collapse);
  return prepare_impl(r);
}

int slg_batch_run(slg_batch *b) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    slg_index *ix = b->idx;
    const IndexState &S = *b->snap;  // the state the batch was prepared on (not the index's current one)
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard g(ix->device);
    hipStream_t st = batch_stream(b);
    b->launched = true;
    b->last_sharded = false;  // (slg_batch_run_sharded* sets it behind this call)
    if (b->nq == 0) return;
    if (b->scan) {
      scan_launch(b, st);  // (no scored term: the candidates come from a scan over the segments' docs)
    } else if (b->n_slices == 0) {
      SLG_HIP(hipMemsetAsync(b->d_q_scored.p, 0, (size_t)b->nq * 4, st));
    } else {
      slg::RoundPartParams pp{};
      pp.sq = b->d_sq;
      pp.terms = b->d_terms;
      pp.n_sq = b->n_sq;
      pp.bnd_coarse = b->d_bnd_coarse;
      pp.segs = S.d_segs.as<slg::SegDev>();
      pp.bounds = b->d_bounds.as<uint32_t>();
      pp.rdoc = b->d_rdoc.as<uint32_t>();
      pp.q_scored = b->d_q_scored.as<uint32_t>();
      const bool skipping = b->d_blk_skip.p != nullptr;
      pp.skip_counts = skipping ? b->d_blk_skip.as<unsigned long long>() : nullptr;
      pp.slice_sq = b->d_slice_sq;
      pp.slice_order = b->d_slice_order;
      pp.slice_desc = b->d_slice_desc.as<slg::SliceDesc>();
      pp.nq = b->nq;
      // the blocked few-term kernel can cut its slices itself (slg_tuning.inline_cuts)
      const bool inline_cuts = b->uniform && (ix->tune.inline_cuts >= 0 ? ix->tune.inline_cuts != 0 : true);
      pp.n_boundaries = inline_cuts ? 0u : b->n_boundaries;
      pp.n_slices = b->n_slices;
      pp.tpb_shift = b->max_terms <= 4 ? 2u : 3u;
      const int score_kind =
          b->uniform ? uniform_kind(b->max_terms, b->plan_batch) : (b->pruned ? 3 : 2);
      const uint64_t pthreads = std::max<uint64_t>(
          std::max<uint64_t>((uint64_t)pp.n_boundaries << pp.tpb_shift, (uint64_t)b->nq + 1), b->n_slices);
      hipLaunchKernelGGL(slg::partition_rounds_kernel, dim3((uint32_t)((pthreads + 255) / 256)),
                         dim3(256), 0, st, pp);
      SLG_HIP(hipGetLastError());

      slg::RoundScoreParams sp{};
      sp.sq = b->d_sq;
      sp.terms = b->d_terms;
      sp.slice_sq = b->d_slice_sq;
      sp.slice_order = b->d_slice_order;
      sp.slice_desc = b->d_slice_desc.as<slg::SliceDesc>();
      sp.reject_table = S.d_reject_table.as<const uint32_t *>();
      sp.n_segs = (uint32_t)S.segs.size();
      sp.plan_batch = b->plan_batch ? (b->deep ? 4u : (b->nested ? 2u : 1u)) : 0u;
      sp.plan_nodes = b->d_nodes;
      sp.cand = b->d_cand.as<uint2>();
      sp.slice_cbeg = b->d_slice_cbeg.as<uint64_t>();
      sp.slice_ccnt = b->d_slice_ccnt.as<uint32_t>();
      sp.segs = S.d_segs.as<slg::SegDev>();
      sp.bounds = inline_cuts ? nullptr : b->d_bounds.as<uint32_t>();
      sp.rdoc = inline_cuts ? nullptr : b->d_rdoc.as<uint32_t>();
      sp.slice_tk = b->d_slice_tk.as<int32_t>();
      sp.slice_doc = b->d_slice_doc.as<uint32_t>();
      sp.q_scored = b->d_q_scored.as<uint32_t>();
      sp.n_slices = b->n_slices;
      sp.k = b->score_k;
      sp.block_skip = skipping ? 1u : 0u;
      sp.skip_counts = pp.skip_counts;
      sp.stamps = nullptr;
      sp.error_flag = ix->d_error_flag.as<uint32_t>();
#ifdef SLG_STAMPS
      b->d_stamps.alloc((size_t)b->n_slices * 96);
      sp.stamps = b->d_stamps.as<unsigned long long>();
#endif
      std::pair<hipEvent_t, hipEvent_t> *ev = nullptr;
      if (ix->profile) {
        if (ix->prof_used == ix->prof_events.size()) {
          hipEvent_t a, c;
          SLG_HIP(hipEventCreate(&a));
          SLG_HIP(hipEventCreate(&c));
          ix->prof_events.emplace_back(a, c);
        }
        ev = &ix->prof_events[ix->prof_used++];
        SLG_HIP(hipEventRecord(ev->first, st));
      }
      launch_score(sp, score_kind, st);
      if (ev) SLG_HIP(hipEventRecord(ev->second, st));
    }
    // (in front of the select: the regions hold accepted candidates only; a phrase batch launches its own
    //  kernel alone, which evaluates the term groups too)
    if (b->phrase) phrase_launch(b, st);
    else if (b->boolean) bool_launch(b, st);
    else if (b->booltree) booltree_launch(b, st);
    // (a script batch: the stage of the inner node first, the outer node reads the score it left)
    if (b->script && b->script_first) script_launch(b, st);
    if (b->fscore) fscore_launch(b, st);  // (the candidates' scores rewritten, those below min_score dropped)
    if (b->script && !b->script_first) script_launch(b, st);
    if (b->sorted) {  // (also without slices: every row is empty, every matched count 0)
      slg::SortedSelectParams sp{};
      fill_select(sp, b);
      sp.sort_cols = b->d_sort_cols.as<const slg::SortColDev>();
      sp.n_parts = b->n_sort_parts;
      sp.score_parts = b->sort_score_parts;
      sp.desc_parts = b->sort_desc_parts;
      if (b->after) {
        hipLaunchKernelGGL(slg::select_sorted_kernel<true>, dim3(b->nq), dim3(slg::kSortedThreads), 0, st, sp);
      } else {
        hipLaunchKernelGGL(slg::select_sorted_kernel<false>, dim3(b->nq), dim3(slg::kSortedThreads), 0, st, sp);
      }
      SLG_HIP(hipGetLastError());
    } else if (b->after || (b->k > 0 && b->cand_mode && b->n_slices > 0)) {
      // (a cursor batch in score order runs the select also without slices or with k = 0: it writes the
      //  matched counts and seen flags)
      slg::SelectParams sp{};
      fill_select(sp, b);
      if (b->after) {
        hipLaunchKernelGGL(slg::select_topk_kernel<true>, dim3(b->nq), dim3(slg::kSelectThreads), 0, st, sp);
      } else {
        hipLaunchKernelGGL(slg::select_topk_kernel<false>, dim3(b->nq), dim3(slg::kSelectThreads), 0, st, sp);
      }
      SLG_HIP(hipGetLastError());
    } else if (b->k > 0 && !b->scan) {
      // (a scan batch comes here only without a slice — no segment has a doc — and has no per-slice top-k lists to
      //  merge: scan_launch zeroed its rows, the counts follow below)
      slg::MergeParams mp{};
      fill_final(mp, b);
      mp.slice_tk = b->d_slice_tk.as<int32_t>();
      mp.slice_doc = b->d_slice_doc.as<uint32_t>();
      launch_merge(mp, st);
    } else {
      SLG_HIP(hipMemsetAsync(b->d_out_count, 0, ((size_t)b->nq + 1) * 4, st));  // (k = 0, or a scan without a slice: no row)
    }
    if (b->aggs) agg_launch(b, st);  // (after the select: the tables of every accepted candidate)
    if (b->top_hits) top_hits_launch(b, st);  // (behind agg_kernel: the parents' count rows are read)
    if (b->composite) composite_launch(b, st);  // (the select, then the collect into the selected rows)
    if (b->term_buckets) term_buckets_launch(b, st);  // (the count walk, the select, the children's collect)
    if (b->rescore) rescore_launch(b, st);  // (behind the rows: the first w of every query are scored again)
    if (b->collapse) collapse_launch(b, st);  // (behind the rows: they are read, never written)
  });
}

int slg_batch_sync(slg_batch *b) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    DeviceGuard g(b->idx->device);
    SLG_HIP(hipStreamSynchronize(batch_stream(b)));
  });
}

int slg_batch_fetch(slg_batch *b, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                    uint32_t *out_count, slg_stats *stats) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->nq == 0 || (out_count != nullptr), "out_count is NULL");
    SLG_REQUIRE(b->nq == 0 || b->k == 0 || (out_doc && out_seg && out_score), "output array is NULL");
    slg_index *ix = b->idx;
    DeviceGuard g(ix->device);
    const hipStream_t st = locked_stream(b);
    const ResultBlock R(b->nq, b->k);
    std::vector<uint32_t> scored;
    std::vector<unsigned long long> skipped;
    if (b->nq) {
      // the results are one contiguous block doc | seg | score | count | error word: ONE D2H copy.
      // Large blocks (config 4: 10 MB) go into a PINNED staging image of the index's pool: a pageable
      // destination makes the runtime stage the copy itself, chunk by chunk behind a lock that every
      // caller thread's copies share.  Small ones (config 2: 46 KB) are copied straight into a pageable
      // image: for them the runtime's own path is the faster one (measured on one box, 8 caller threads,
      // 20-step regions: 12.1-12.5M against 10.4-11.0M queries/s with the pinned image and a separate
      // 4-byte copy of the error word).
      const size_t words = R.words_with_flag();
      const size_t extra = stats ? (size_t)b->nq + ((b->d_blk_skip.p && b->launched) ? 2 * ((size_t)b->nq + 1) : 0) : 0;
      FetchBlock host(ix->pool, words + extra);
      uint32_t *const blk = host.p;
      SLG_HIP(hipMemcpyAsync(blk, b->d_out.p, words * 4, hipMemcpyDeviceToHost, st));
      uint32_t *flagw = R.flag(blk);  // the index's error word as the batch's last kernel saw it
      uint32_t *const sblk = blk + words;
      if (stats) {
        SLG_HIP(hipMemcpyAsync(sblk, b->d_q_scored.p, (size_t)b->nq * 4, hipMemcpyDeviceToHost, st));
        if (b->d_blk_skip.p && b->launched)
          SLG_HIP(hipMemcpyAsync(sblk + b->nq, b->d_blk_skip.p, ((size_t)b->nq + 1) * 8, hipMemcpyDeviceToHost, st));
      }
      SLG_HIP(wait_stream(st));
      if (*flagw != 0u)
        throw SlgError(SLG_ERR_INTERNAL, "a scoring wave gave up on a round (chunk-loop guard): results are incomplete");
      R.unpack(blk, out_doc, out_seg, out_score, out_count);
      if (stats) {
        scored.assign(sblk, sblk + b->nq);
        if (b->d_blk_skip.p && b->launched) {
          skipped.resize((size_t)b->nq + 1);
          std::memcpy(skipped.data(), sblk + b->nq, skipped.size() * 8);
        }
      }
    }
    if (stats)
      for (uint32_t q = 0; q < b->nq; q++) {
        // brute-force accounting: wand.rs:472 (postings_advanced += len), :500-503; with block
        // skipping, the postings that were never loaded are not counted as advanced over
        stats[q].postings_advanced = b->q_postings[q] - (skipped.empty() ? 0ull : skipped[q + 1]);
        stats[q].scored_docs = scored[q];
        stats[q].candidates_examined = scored[q];
      }
  });
}

int slg_batch_device_results(slg_batch *b, void **d_doc, void **d_seg, void **d_score,
                             void **d_count) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    if (d_doc) *d_doc = b->d_out_doc;
    if (d_seg) *d_seg = b->d_out_seg;
    if (d_score) *d_score = b->d_out_score;
    if (d_count) *d_count = b->d_out_count;
  });
}

int slg_batch_device_result_block(slg_batch *b, void **d_block, uint64_t *n_bytes) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    if (d_block) *d_block = b->d_out.p;
    if (n_bytes) *n_bytes = (uint64_t)ResultBlock(b->nq, b->k).words() * 4;
  });
}

int slg_batch_info(const slg_batch *b, uint64_t *n_postings, uint32_t *n_slices,
                   uint64_t *algorithmic_bytes) {
  return guarded([&] {
    SLG_REQUIRE(b != nullptr, "batch is NULL");
    if (n_postings) *n_postings = b->n_postings;
    if (n_slices) *n_slices = b->n_slices;
    if (algorithmic_bytes) *algorithmic_bytes = 12ull * b->n_postings + 8ull * b->k * b->nq;
  });
}

int slg_batch_skip_counts(slg_batch *b, uint64_t *probed_postings, uint64_t *skipped_postings) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    DeviceGuard g(b->idx->device);
    unsigned long long c = 0ull;
    if (b->d_blk_skip.p) {
      SLG_HIP(hipStreamSynchronize(batch_stream(b)));
      SLG_HIP(hipMemcpy(&c, b->d_blk_skip.p, 8, hipMemcpyDeviceToHost));
    }
    if (probed_postings) *probed_postings = b->d_blk_skip.p ? b->n_postings_nonessential : 0ull;
    if (skipped_postings) *skipped_postings = c;
  });
}

#ifdef SLG_STAMPS
int slg_debug_read_stamps(slg_batch *b, unsigned long long *out, uint32_t n_slices) {
  return guarded([&] {
    SLG_HIP(hipStreamSynchronize(batch_stream(b)));
    SLG_HIP(hipMemcpy(out, b->d_stamps.p, (size_t)n_slices * 96, hipMemcpyDeviceToHost));
  });
}
#endif

int slg_batch_set_stream(slg_batch *b, void *hip_stream) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    slg_index *ix = b->idx;
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard g(ix->device);
    if (b->launched) SLG_HIP(hipStreamSynchronize(batch_stream(b)));  // queued work finishes first
    b->own_stream_set = hip_stream != SLG_OWN_STREAM;
    b->stream = b->own_stream_set ? (hipStream_t)hip_stream : nullptr;
  });
}

void slg_batch_destroy(slg_batch *b) {
  if (!b) return;
  slg_index *ix = b->idx;
  if (!ix) {  // detached by slg_index_destroy: nothing left on the device, the shard events gone too
    delete b;
    return;
  }
  DeviceScope on(ix->device);
  hipStream_t st;
  {
    std::lock_guard<std::mutex> lk(ix->mu);
    st = batch_stream(b);
    auto it = std::find(ix->live.begin(), ix->live.end(), b);
    if (it != ix->live.end()) {
      *it = ix->live.back();
      ix->live.pop_back();
    }
  }
  (void)wait_stream(st);
  for (hipEvent_t e : b->ev_shard)
    if (e) (void)hipEventDestroy(e);
  delete b;
}

}  // extern "C"

namespace {
// slg_query[] as the flat arrays of slg_batch_prepare*: offsets, term ids (one row of n_segs per term), weights
struct FlatQueries {
  std::vector<uint32_t> offs, tids;
  std::vector<float> ws;
};
int flatten_queries(slg_index *ix, const slg_query *queries, uint32_t nq, FlatQueries *fq) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(nq == 0 || queries != nullptr, "queries is NULL");
    const size_t n_segs = ix->snapshot()->segs.size();
    fq->offs.assign((size_t)nq + 1, 0u);
    for (uint32_t q = 0; q < nq; q++) {
      const slg_query &qq = queries[q];
      SLG_REQUIRE(qq.n_terms == 0 || (qq.term_ids && qq.weights), "query arrays are NULL");
      fq->offs[q + 1] = fq->offs[q] + qq.n_terms;
      fq->tids.insert(fq->tids.end(), qq.term_ids, qq.term_ids + (size_t)qq.n_terms * n_segs);
      fq->ws.insert(fq->ws.end(), qq.weights, qq.weights + qq.n_terms);
    }
  });
}

}  // namespace

int slghost::run_to_host(slg_batch *b, const HostOut &o) {
  if (!b) return last_error().code;
  int rc = slg_batch_run(b);
  if (rc == SLG_OK) rc = slg_batch_fetch(b, o.doc, o.seg, o.score, o.count, o.stats);
  if (rc == SLG_OK && o.matched) rc = slg_batch_matched_counts(b, o.matched);
  if (rc == SLG_OK && (b->aggs || b->composite || b->term_buckets)) rc = slg_batch_fetch_aggs(b, o.agg_counts, o.agg_stats);
  if (rc == SLG_OK && b->composite) rc = slg_batch_fetch_composite(b, o.cp_keys, o.cp_n_buckets, o.cp_has_more);
  if (rc == SLG_OK && b->term_buckets)
    rc = slg_batch_fetch_term_buckets(b, o.tb_ords, o.tb_doc_counts, o.tb_bg_counts, o.tb_score_bits, o.tb_n_buckets,
                                      o.tb_node_dc, o.tb_node_bg);
  if (rc == SLG_OK && b->aggs && b->agg_value_nodes) rc = slg_batch_fetch_agg_values(b, o.agg_values);
  if (rc == SLG_OK && b->top_hits) rc = slg_batch_fetch_top_hits(b, o.th_doc, o.th_seg, o.th_score, o.th_count, o.th_status);
  if (rc == SLG_OK && b->rescore) rc = slg_batch_fetch_rescore(b, o.first_score, o.rescore_score, o.rescored);
  if (rc == SLG_OK && o.seen) rc = slg_batch_cursor_seen(b, o.seen);
  if (rc == SLG_OK && b->collapse) {
    void *const *c = o.collapse;
    auto u = [c](int i) { return static_cast<uint32_t *>(c[i]); };
    rc = slg_batch_fetch_collapse(b, u(0), u(1), u(2), u(3), u(4), u(5), u(6), u(7), static_cast<float *>(c[8]), u(9),
                                  u(10), u(11), u(12), static_cast<float *>(c[13]));
  }
  KeepLastError keep;
  slg_batch_destroy(b);
  return rc;
}

extern "C" {

int slg_search_batch(slg_index *ix, const slg_query *queries, uint32_t nq, uint32_t k,
                     int strategy, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                     uint32_t *out_count, slg_stats *stats) {
  return slg_search_batch_filtered(ix, queries, nq, nullptr, k, strategy, out_doc, out_seg, out_score,
                                   out_count, stats);
}

int slg_search_batch_filtered(slg_index *ix, const slg_query *queries, uint32_t nq,
                              const int32_t *q_filter, uint32_t k, int strategy, uint32_t *out_doc,
                              uint32_t *out_seg, float *out_score, uint32_t *out_count,
                              slg_stats *stats) {
  FlatQueries fq;
  const int rc = flatten_queries(ix, queries, nq, &fq);
  if (rc != SLG_OK) return rc;
  return run_to_host(slg_batch_prepare_filtered(ix, nq, fq.offs.data(), fq.tids.data(), fq.ws.data(), q_filter, k,
                                                strategy),
                     HostOut{out_doc, out_seg, out_score, out_count, stats});
}

int slg_batch_matched_counts(slg_batch *b, uint64_t *out_matched) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    if (b->hybrid) throw SlgError(SLG_ERR_UNSUPPORTED, "a hybrid batch has no matched counts");
    SLG_REQUIRE(b->d_matched.p != nullptr,
                "not a sorted, cursor, aggregation or scan batch (slg_batch_prepare_sorted / _after / _aggs / _scan)");
    SLG_REQUIRE(b->launched, "the batch has not run");
    SLG_REQUIRE(b->nq == 0 || out_matched != nullptr, "out_matched is NULL");
    DeviceGuard g(b->idx->device);
    SLG_HIP(wait_stream(locked_stream(b)));
    if (b->nq) SLG_HIP(hipMemcpy(out_matched, b->d_matched.p, (size_t)b->nq * 8, hipMemcpyDeviceToHost));
  });
}

int slg_search_batch_sorted(slg_index *ix, const slg_query *queries, uint32_t nq, const slg_score_plans *plans,
                            const int32_t *q_filter, const slg_sort_spec *sort, uint32_t k, int strategy,
                            uint32_t *out_doc, uint32_t *out_seg, float *out_score, uint32_t *out_count,
                            uint64_t *out_matched) {
  FlatQueries fq;
  const int rc = flatten_queries(ix, queries, nq, &fq);
  if (rc != SLG_OK) return rc;
  return run_to_host(slg_batch_prepare_sorted(ix, nq, fq.offs.data(), fq.tids.data(), fq.ws.data(), plans, q_filter,
                                              sort, k, strategy),
                     HostOut{out_doc, out_seg, out_score, out_count, nullptr, out_matched});
}

slg_batch *slg_batch_prepare_aggs(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                                  const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                                  const slg_sort_spec *sort, const slg_agg_spec *aggs, uint32_t k, int strategy) {
  PrepareRequest r{ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy};
  r.sort = if_given(sort);
  r.aggs = {true, aggs};
  return prepare_impl(r);
}

int slg_search_batch_agg_values(slg_index *ix, const slg_query *queries, uint32_t nq, const slg_score_plans *plans,
                                const int32_t *q_filter, const slg_sort_spec *sort, const slg_agg_spec *aggs, uint32_t k,
                                int strategy, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                                uint32_t *out_count, uint64_t *out_matched, uint64_t *counts, slg_agg_stats *stats,
                                uint64_t *values) {
  FlatQueries fq;
  const int rc = flatten_queries(ix, queries, nq, &fq);
  if (rc != SLG_OK) return rc;
  HostOut o{out_doc, out_seg, out_score, out_count, nullptr, out_matched, nullptr, counts, stats};
  o.agg_values = values;
  return run_to_host(slg_batch_prepare_aggs(ix, nq, fq.offs.data(), fq.tids.data(), fq.ws.data(), plans, q_filter,
                                            sort, aggs, k, strategy),
                     o);
}

int slg_search_batch_aggs(slg_index *ix, const slg_query *queries, uint32_t nq, const slg_score_plans *plans,
                          const int32_t *q_filter, const slg_sort_spec *sort, const slg_agg_spec *aggs, uint32_t k,
                          int strategy, uint32_t *out_doc, uint32_t *out_seg, float *out_score, uint32_t *out_count,
                          uint64_t *out_matched, uint64_t *counts, slg_agg_stats *stats) {
  // this form has nowhere to put a value table: it refuses the spec and drops nothing silently
  const int rc = guarded([&] {
    for (uint32_t i = 0; aggs && i < aggs->n_nodes && i < SLG_MAX_AGGS; i++)
      SLG_REQUIRE(aggs->nodes[i].kind < SLG_AGG_CARDINALITY || aggs->nodes[i].kind > SLG_AGG_PERCENTILE_RANKS,
                  "agg node " + std::to_string(i) + " has a value table: use slg_search_batch_agg_values");
  });
  if (rc != SLG_OK) return rc;
  return slg_search_batch_agg_values(ix, queries, nq, plans, q_filter, sort, aggs, k, strategy, out_doc, out_seg,
                                     out_score, out_count, out_matched, counts, stats, nullptr);
}

slg_batch *slg_batch_prepare_top_hits(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                                      const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                                      const slg_sort_spec *sort, const slg_agg_spec *aggs,
                                      const slg_top_hits_spec *top_hits, uint32_t k, int strategy) {
  PrepareRequest r{ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy};
  r.sort = if_given(sort);
  r.aggs = if_given(aggs);
  r.top_hits = {true, top_hits};
  return prepare_impl(r);
}

int slg_search_batch_top_hits(slg_index *ix, const slg_query *queries, uint32_t nq, const slg_score_plans *plans,
                              const int32_t *q_filter, const slg_sort_spec *sort, const slg_agg_spec *aggs,
                              const slg_top_hits_spec *top_hits, uint32_t k, int strategy, uint32_t *out_doc,
                              uint32_t *out_seg, float *out_score, uint32_t *out_count, uint64_t *out_matched,
                              uint64_t *counts, slg_agg_stats *stats, uint64_t *values, uint32_t *th_doc,
                              uint32_t *th_seg, float *th_score, uint32_t *th_count, uint32_t *th_status) {
  FlatQueries fq;
  const int rc = flatten_queries(ix, queries, nq, &fq);
  if (rc != SLG_OK) return rc;
  HostOut o{out_doc, out_seg, out_score, out_count, nullptr, out_matched, nullptr, counts, stats};
  o.agg_values = values;
  o.th_doc = th_doc;
  o.th_seg = th_seg;
  o.th_score = th_score;
  o.th_count = th_count;
  o.th_status = th_status;
  return run_to_host(slg_batch_prepare_top_hits(ix, nq, fq.offs.data(), fq.tids.data(), fq.ws.data(), plans, q_filter,
                                                sort, aggs, top_hits, k, strategy),
                     o);
}

slg_batch *slg_batch_prepare_composite(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                                       const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                                       const slg_sort_spec *sort, const slg_agg_spec *aggs,
                                       const slg_composite_spec *composite, uint32_t k, int strategy) {
  PrepareRequest r{ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy};
  r.sort = if_given(sort);
  r.aggs = if_given(aggs);
  r.composite = {true, composite};
  return prepare_impl(r);
}

int slg_search_batch_composite(slg_index *ix, const slg_query *queries, uint32_t nq, const slg_score_plans *plans,
                               const int32_t *q_filter, const slg_sort_spec *sort, const slg_agg_spec *aggs,
                               const slg_composite_spec *composite, uint32_t k, int strategy, uint32_t *out_doc,
                               uint32_t *out_seg, float *out_score, uint32_t *out_count, uint64_t *out_matched,
                               uint64_t *counts, slg_agg_stats *stats, uint64_t *cp_keys, uint32_t *cp_n_buckets,
                               uint32_t *cp_has_more) {
  FlatQueries fq;
  const int rc = flatten_queries(ix, queries, nq, &fq);
  if (rc != SLG_OK) return rc;
  HostOut o{out_doc, out_seg, out_score, out_count, nullptr, out_matched, nullptr, counts, stats};
  o.cp_keys = cp_keys;
  o.cp_n_buckets = cp_n_buckets;
  o.cp_has_more = cp_has_more;
  return run_to_host(slg_batch_prepare_composite(ix, nq, fq.offs.data(), fq.tids.data(), fq.ws.data(), plans, q_filter,
                                                 sort, aggs, composite, k, strategy),
                     o);
}

slg_batch *slg_batch_prepare_term_buckets(slg_index *ix, uint32_t nq, const uint32_t *q_offsets,
                                          const uint32_t *q_term_ids, const float *q_weights,
                                          const slg_score_plans *plans, const int32_t *q_filter,
                                          const slg_sort_spec *sort, const slg_agg_spec *aggs,
                                          const slg_term_bucket_spec *spec, uint32_t k, int strategy) {
  PrepareRequest r{ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy};
  r.sort = if_given(sort);
  r.aggs = if_given(aggs);
  r.term_buckets = {true, spec};
  return prepare_impl(r);
}

int slg_search_batch_term_buckets(slg_index *ix, const slg_query *queries, uint32_t nq, const slg_score_plans *plans,
                                  const int32_t *q_filter, const slg_sort_spec *sort, const slg_agg_spec *aggs,
                                  const slg_term_bucket_spec *spec, uint32_t k, int strategy, uint32_t *out_doc,
                                  uint32_t *out_seg, float *out_score, uint32_t *out_count, uint64_t *out_matched,
                                  uint64_t *counts, slg_agg_stats *stats, uint32_t *tb_ords, uint64_t *tb_doc_counts,
                                  uint64_t *tb_bg_counts, uint64_t *tb_score_bits, uint32_t *tb_n_buckets,
                                  uint64_t *tb_node_doc_count, uint64_t *tb_node_bg_count) {
  FlatQueries fq;
  const int rc = flatten_queries(ix, queries, nq, &fq);
  if (rc != SLG_OK) return rc;
  HostOut o{out_doc, out_seg, out_score, out_count, nullptr, out_matched, nullptr, counts, stats};
  o.tb_ords = tb_ords;
  o.tb_doc_counts = tb_doc_counts;
  o.tb_bg_counts = tb_bg_counts;
  o.tb_score_bits = tb_score_bits;
  o.tb_n_buckets = tb_n_buckets;
  o.tb_node_dc = tb_node_doc_count;
  o.tb_node_bg = tb_node_bg_count;
  return run_to_host(slg_batch_prepare_term_buckets(ix, nq, fq.offs.data(), fq.tids.data(), fq.ws.data(), plans,
                                                    q_filter, sort, aggs, spec, k, strategy),
                     o);
}

slg_batch *slg_batch_prepare_rescore(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                                     const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                                     const slg_rescore_spec *rescore, uint32_t k, int strategy) {
  PrepareRequest r{ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy};
  r.rescore = {true, rescore};
  return prepare_impl(r);
}

int slg_search_batch_rescore(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                             const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                             const slg_rescore_spec *rescore, uint32_t k, int strategy, uint32_t *out_doc,
                             uint32_t *out_seg, float *out_score, uint32_t *out_count, float *out_first_score,
                             float *out_rescore_score, uint32_t *out_rescored) {
  HostOut o{out_doc, out_seg, out_score, out_count};
  o.first_score = out_first_score;
  o.rescore_score = out_rescore_score;
  o.rescored = out_rescored;
  return run_to_host(slg_batch_prepare_rescore(ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, rescore, k,
                                               strategy),
                     o);
}

slg_batch *slg_batch_prepare_bool(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                                  const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                                  const slg_sort_spec *sort, const slg_bool_spec *spec, uint32_t k, int strategy) {
  PrepareRequest r{ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy};
  r.sort = if_given(sort);
  r.boolean = {true, spec};
  return prepare_impl(r);
}

int slg_search_batch_bool(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                          const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                          const slg_sort_spec *sort, const slg_bool_spec *spec, uint32_t k, int strategy,
                          uint32_t *out_doc, uint32_t *out_seg, float *out_score, uint32_t *out_count,
                          slg_stats *stats, uint64_t *out_matched) {
  return run_to_host(slg_batch_prepare_bool(ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, sort, spec, k,
                                            strategy),
                     HostOut{out_doc, out_seg, out_score, out_count, stats, out_matched});
}

slg_batch *slg_batch_prepare_bool_tree(slg_index *ix, uint32_t nq, const uint32_t *q_offsets,
                                       const uint32_t *q_term_ids, const float *q_weights,
                                       const slg_score_plans *plans, const int32_t *q_filter,
                                       const slg_sort_spec *sort, const slg_bool_tree_spec *spec, uint32_t k,
                                       int strategy) {
  PrepareRequest r{ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy};
  r.sort = if_given(sort);
  r.booltree = {true, spec};
  return prepare_impl(r);
}

int slg_search_batch_bool_tree(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                               const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                               const slg_sort_spec *sort, const slg_bool_tree_spec *spec, uint32_t k, int strategy,
                               uint32_t *out_doc, uint32_t *out_seg, float *out_score, uint32_t *out_count,
                               slg_stats *stats, uint64_t *out_matched) {
  return run_to_host(slg_batch_prepare_bool_tree(ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, sort, spec,
                                                 k, strategy),
                     HostOut{out_doc, out_seg, out_score, out_count, stats, out_matched});
}

slg_batch *slg_batch_prepare_phrase(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                                    const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                                    const slg_sort_spec *sort, const slg_bool_spec *boolean,
                                    const slg_phrase_spec *phrases, uint32_t k, int strategy) {
  PrepareRequest r{ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy};
  r.sort = if_given(sort);
  r.boolean = {true, boolean};  // (NULL: the batch has no term groups)
  r.phrase = {true, phrases};
  return prepare_impl(r);
}

int slg_search_batch_phrase(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                            const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                            const slg_sort_spec *sort, const slg_bool_spec *boolean, const slg_phrase_spec *phrases,
                            uint32_t k, int strategy, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                            uint32_t *out_count, slg_stats *stats, uint64_t *out_matched) {
  return run_to_host(slg_batch_prepare_phrase(ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, sort,
                                              boolean, phrases, k, strategy),
                     HostOut{out_doc, out_seg, out_score, out_count, stats, out_matched});
}

slg_batch *slg_batch_prepare_fscore(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                                    const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                                    const slg_sort_spec *sort, const slg_fscore_spec *spec, uint32_t k, int strategy) {
  PrepareRequest r{ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy};
  r.sort = if_given(sort);
  r.fscore = {true, spec};
  return prepare_impl(r);
}

int slg_search_batch_fscore(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                            const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                            const slg_sort_spec *sort, const slg_fscore_spec *spec, uint32_t k, int strategy,
                            uint32_t *out_doc, uint32_t *out_seg, float *out_score, uint32_t *out_count,
                            slg_stats *stats, uint64_t *out_matched) {
  return run_to_host(slg_batch_prepare_fscore(ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, sort, spec, k,
                                              strategy),
                     HostOut{out_doc, out_seg, out_score, out_count, stats, out_matched});
}

slg_batch *slg_batch_prepare_script(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                                    const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                                    const slg_sort_spec *sort, const slg_script_spec *script,
                                    const slg_fscore_spec *fscore, int order, uint32_t k, int strategy) {
  PrepareRequest r{ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy};
  r.sort = if_given(sort);
  r.fscore = if_given(fscore);
  r.script = {true, script};
  r.script_order = order;
  return prepare_impl(r);
}

int slg_search_batch_script(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                            const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                            const slg_sort_spec *sort, const slg_script_spec *script, const slg_fscore_spec *fscore,
                            int order, uint32_t k, int strategy, uint32_t *out_doc, uint32_t *out_seg,
                            float *out_score, uint32_t *out_count, slg_stats *stats, uint64_t *out_matched) {
  return run_to_host(slg_batch_prepare_script(ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, sort, script,
                                              fscore, order, k, strategy),
                     HostOut{out_doc, out_seg, out_score, out_count, stats, out_matched});
}

slg_batch *slg_batch_prepare_collapse(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                                      const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                                      const slg_sort_spec *sort, const slg_sort_cursor *q_cursor,
                                      const slg_collapse_spec *collapse, uint32_t k, int strategy) {
  PrepareRequest r{ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, k, strategy};
  r.sort = if_given(sort);
  r.cursor = if_given(q_cursor);
  r.collapse = {true, collapse};
  return prepare_impl(r);
}

int slg_search_batch_collapse(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                              const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                              const slg_sort_spec *sort, const slg_sort_cursor *q_cursor,
                              const slg_collapse_spec *collapse, uint32_t k, int strategy, uint32_t *out_doc,
                              uint32_t *out_seg, float *out_score, uint32_t *out_count, uint32_t *n_groups,
                              uint32_t *total_groups, uint32_t *status, uint32_t *group_row, uint32_t *group_ord,
                              uint32_t *group_size, uint32_t *group_doc, uint32_t *group_seg, float *group_score,
                              uint32_t *inner_count, uint32_t *inner_row, uint32_t *inner_doc, uint32_t *inner_seg,
                              float *inner_score) {
  void *const arrays[14] = {n_groups,  total_groups, status,      group_row, group_ord, group_size, group_doc,
                            group_seg, group_score,  inner_count, inner_row, inner_doc, inner_seg,  inner_score};
  HostOut o{out_doc, out_seg, out_score, out_count};
  o.collapse = arrays;
  return run_to_host(slg_batch_prepare_collapse(ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, sort,
                                                q_cursor, collapse, k, strategy),
                     o);
}

int slg_batch_cursor_seen(slg_batch *b, uint8_t *out_seen) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    if (b->hybrid) throw SlgError(SLG_ERR_UNSUPPORTED, "a hybrid batch takes no cursor");
    SLG_REQUIRE(b->after, "not a cursor batch (slg_batch_prepare_after)");
    SLG_REQUIRE(b->launched, "the batch has not run");
    SLG_REQUIRE(b->nq == 0 || out_seen != nullptr, "out_seen is NULL");
    DeviceGuard g(b->idx->device);
    SLG_HIP(wait_stream(locked_stream(b)));
    std::vector<uint32_t> seen(b->nq);
    if (b->nq) SLG_HIP(hipMemcpy(seen.data(), b->d_seen.p, (size_t)b->nq * 4, hipMemcpyDeviceToHost));
    for (uint32_t q = 0; q < b->nq; q++) out_seen[q] = seen[q] ? 1u : 0u;
  });
}

int slg_search_batch_after(slg_index *ix, const slg_query *queries, uint32_t nq, const slg_score_plans *plans,
                           const int32_t *q_filter, const slg_sort_spec *sort, const slg_sort_cursor *q_cursor,
                           uint32_t k, int strategy, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                           uint32_t *out_count, uint64_t *out_matched, uint8_t *out_seen) {
  FlatQueries fq;
  const int rc = flatten_queries(ix, queries, nq, &fq);
  if (rc != SLG_OK) return rc;
  return run_to_host(slg_batch_prepare_after(ix, nq, fq.offs.data(), fq.tids.data(), fq.ws.data(), plans, q_filter,
                                             sort, q_cursor, k, strategy),
                     HostOut{out_doc, out_seg, out_score, out_count, nullptr, out_matched, out_seen});
}

int slg_merge_shards_device(slg_index *ix, uint32_t n_shards, uint32_t nq, uint32_t k,
                            const uint32_t *d_doc, const uint32_t *d_seg, const float *d_score,
                            const uint32_t *d_count, uint32_t seg_stride, uint32_t *d_out_doc,
                            uint32_t *d_out_seg, float *d_out_score, uint32_t *d_out_count) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    if (k > SLG_MAX_K) throw SlgError(SLG_ERR_UNSUPPORTED, "k > SLG_MAX_K");
    if (nq == 0) return;
    SLG_REQUIRE(n_shards >= 1, "n_shards == 0");
    SLG_REQUIRE(d_count && d_out_count, "count arrays are NULL");
    SLG_REQUIRE(k == 0 || (d_doc && d_seg && d_score && d_out_doc && d_out_seg && d_out_score),
                "device arrays are NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard g(ix->device);
    if (k == 0) {
      SLG_HIP(hipMemsetAsync(d_out_count, 0, (size_t)nq * 4, ix->stream));
      return;
    }
    slg::ShardMergeParams mp{};
    mp.doc = d_doc;
    mp.seg = d_seg;
    mp.score = d_score;
    mp.count = d_count;
    mp.out_doc = d_out_doc;
    mp.out_seg = d_out_seg;
    mp.out_score = d_out_score;
    mp.out_count = d_out_count;
    mp.n_shards = n_shards;
    mp.nq = nq;
    mp.k = k;
    mp.seg_stride = seg_stride;
    mp.arr_stride = (uint64_t)nq * k;
    mp.cnt_stride = nq;
    launch_shard_merge(mp, ix->stream);
  });
}

}  // extern "C"
