// slg_tophits.hip — top_hits batches (slg_batch_prepare_top_hits): the spec against the batch's index state and
// its aggregation layout, the node table, sort columns, output arrays and run scratch on the device, the launch of
// top_hits_kernel behind agg_kernel, and slg_batch_top_hits_layout / _fetch_top_hits.  (The checks of a spec that
// need no index: slg_plan.cpp, check_top_hits.)
#include "slg_host.hpp"

#include "slg_tophits.hpp"

using namespace slghost;

static_assert(slg::kTopHitsMaxNodes == SLG_MAX_TOP_HITS_NODES && slg::kTopHitsMaxList == SLG_MAX_TOP_HITS,
              "the kernel's limits and the ABI's");
static_assert(slg::kSortMaxParts == SLG_MAX_SORT_PARTS, "the nodes' sort parts");
static_assert(sizeof(slg::TopHitsNodeDev) == 48, "records the kernel reads in whole words");

namespace {
size_t out_off(const slg_batch *b, uint32_t i) { return slg::top_hits_out(i, b->nq, b->th_hit_cells, b->th_list_cells); }
}  // namespace

void slghost::top_hits_attach(slg_batch *b, const slg_top_hits_spec &spec) {
  const IndexState &S = *b->snap;
  slg_index *ix = b->idx;
  const uint32_t nn = spec.n_nodes;
  std::vector<slg::TopHitsNodeDev> nodes(nn);
  std::vector<slg::SortColDev> cols;
  b->th_layout.assign(nn, slg_top_hits_layout{});
  uint64_t hit_cells = 0, list_cells = 0;
  uint32_t cursor_words = 0, lds_cursors = 0;
  bool ext = false;
  int32_t last_many_parent = -1;  // the parent whose runs the kernel holds when it reaches the node
  for (uint32_t i = 0; i < nn; i++) {
    const slg_top_hits_node &n = spec.nodes[i];
    const std::string name = "top_hits node " + std::to_string(i) + ": ";
    // an empty sort is `_score` desc (query/sort.rs:159-167)
    const slg_sort_spec sort = n.sort.n_parts ? n.sort : slg_sort_spec{1, {SLG_SORT_SCORE}, {SLG_ORDER_DESC}};
    const SortBinding sorting = bind_sort(S, sort, name, "sort part ");
    cols.insert(cols.end(), sorting.cols.begin(), sorting.cols.end());
    slg::TopHitsNodeDev &d = nodes[i];
    d = slg::TopHitsNodeDev{};
    d.parent = n.parent;
    d.from = n.from;
    d.size = n.size;
    d.n_parts = sort.n_parts;
    d.score_parts = sorting.score_parts;
    d.desc_parts = sorting.desc_parts;
    d.lists = 1;
    d.first = 1;
    if (n.parent >= 0) {
      const int32_t kind = b->agg_spec.nodes[n.parent].kind;
      ext = ext || kind == SLG_AGG_DATE_HISTOGRAM || kind == SLG_AGG_FILTER;
      d.many = kind != SLG_AGG_FILTER ? 1u : 0u;
      d.lists = b->agg_layout[n.parent].rows;
      // a query has ONE cursor region and ONE run region: a node finds its parent's runs there only when the
      // many-lists node before it (one-list nodes in between touch neither) had the same parent; else it builds them
      // again, so nodes of one parent that are not adjacent in the spec cost a fill each and are still right
      if (d.many) {
        d.first = last_many_parent == n.parent ? 0u : 1u;
        last_many_parent = n.parent;
      }
      if (d.many && d.first) {
        if (d.lists <= slg::kTopHitsLdsLists) lds_cursors = std::max(lds_cursors, d.lists);
        else cursor_words = std::max(cursor_words, d.lists);
      }
    }
    d.list_off = (uint32_t)list_cells;
    d.hit_off = (uint32_t)hit_cells;
    hit_cells += (uint64_t)d.lists * d.size;
    list_cells += d.lists;
    if (hit_cells > SLG_MAX_TOP_HITS_CELLS)
      throw SlgError(SLG_ERR_UNSUPPORTED, "more than SLG_MAX_TOP_HITS_CELLS hit cells per query (at top_hits node " +
                                              std::to_string(i) + ")");
    b->th_layout[i] = slg_top_hits_layout{d.lists, d.size, d.list_off, d.hit_off};
  }
  b->top_hits = true;
  b->th_spec = spec;
  b->th_hit_cells = (uint32_t)hit_cells;
  b->th_list_cells = (uint32_t)list_cells;
  b->th_max_entries = spec.max_entries ? spec.max_entries : SLG_MAX_TOP_HITS_ENTRIES;
  b->th_cursor_words = cursor_words;
  b->th_lds_cursors = lds_cursors;
  b->th_ext = ext;
  bool many = false;
  for (const slg::TopHitsNodeDev &d : nodes) many = many || d.many;
  upload_image(b->d_th_desc, &ix->pool, {image_part(nodes), image_part(cols)});
  const size_t nq = std::max<uint32_t>(b->nq, 1);
  b->d_th_out.alloc_pooled(&ix->pool, (out_off(b, 5) + 1) * 4);
  if (many) b->d_th_entries.alloc_pooled(&ix->pool, nq * (size_t)b->th_max_entries * 8);
  if (cursor_words) b->d_th_cursors.alloc_pooled(&ix->pool, nq * (size_t)cursor_words * 4);
}

void slghost::top_hits_launch(slg_batch *b, hipStream_t st) {
  if (b->nq == 0) return;
  slg::TopHitsParams p{};
  fill_candidates(p, b);
  const uint32_t an = b->aggs ? b->agg_spec.n_nodes : 0u;
  p.nodes = b->aggs ? b->d_agg_desc.as<const slg::AggNodeDev>() : nullptr;
  p.cols = b->aggs ? reinterpret_cast<const slg::ColumnDev *>(b->d_agg_desc.as<unsigned char>() +
                                                              (size_t)an * sizeof(slg::AggNodeDev))
                   : nullptr;
  p.nq = b->nq;
  p.count_cells = agg_spec_cells(b).count;
  p.counts = b->aggs ? b->d_agg_counts.as<const uint32_t>() : nullptr;
  p.n_th = b->th_spec.n_nodes;
  p.th = b->d_th_desc.as<const slg::TopHitsNodeDev>();
  p.sort_cols = reinterpret_cast<const slg::SortColDev *>(p.th + p.n_th);
  p.match_only = (b->sorted && b->sort_score_parts == 0u) ? 1u : 0u;
  p.max_entries = b->th_max_entries;
  p.cursor_words = b->th_cursor_words;
  p.entries = b->d_th_entries.as<uint2>();
  p.cursors = b->d_th_cursors.as<uint32_t>();
  p.hit_cells = b->th_hit_cells;
  p.list_cells = b->th_list_cells;
  p.out = b->d_th_out.as<uint32_t>();
  p.flag = ResultBlock(b->nq, b->k).flag(b->d_out.as<uint32_t>());
  // a sorted batch's select counted the accepted docs, agg_kernel does in score order; without either this kernel
  p.out_matched = post_select_matched(b);
  const size_t lds = ((size_t)slg::kTopHitsMergeWords + b->th_lds_cursors) * 4;
  launch_kernel_lds(b->th_ext ? slg::top_hits_kernel<true> : slg::top_hits_kernel<false>, p, dim3(b->nq),
                    slg::kTopHitsThreads, lds, st);
}

extern "C" {

int slg_batch_top_hits_layout(const slg_batch *b, slg_top_hits_layout *out) {
  return guarded([&] {
    SLG_REQUIRE(b != nullptr, "batch is NULL");
    SLG_REQUIRE(b->top_hits, "not a top_hits batch (slg_batch_prepare_top_hits)");
    SLG_REQUIRE(out != nullptr, "out is NULL");
    std::copy(b->th_layout.begin(), b->th_layout.end(), out);
  });
}

int slg_batch_fetch_top_hits(slg_batch *b, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                             uint32_t *out_count, uint32_t *out_status) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->top_hits, "not a top_hits batch (slg_batch_prepare_top_hits)");
    SLG_REQUIRE(b->launched, "the batch has not run");
    DeviceGuard g(b->idx->device);
    const hipStream_t st = locked_stream(b);
    if (b->nq == 0) return;
    // the arrays and the error word behind them are one block
    const size_t words = out_off(b, 5) + 1;
    const SideBlock host(b, b->d_th_out, words, st);
    const uint32_t *const blk = host.p;
    void *const dst[5] = {out_doc, out_seg, out_score, out_count, out_status};
    for (uint32_t i = 0; i < 5; i++) {
      const size_t n = out_off(b, i + 1) - out_off(b, i);
      if (dst[i] && n) std::memcpy(dst[i], blk + out_off(b, i), n * 4);
    }
  });
}

}  // extern "C"
