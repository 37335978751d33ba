// slg_collapse.hip — collapse batches (slg_batch_prepare_collapse): the spec against the batch's index state,
// the column tables and side arrays on the device, the launch of collapse_kernel behind the batch's rows, and
// slg_batch_fetch_collapse.  (The checks of a spec that need no index: slg_plan.cpp, check_collapse.)
#include "slg_host.hpp"

#include <optional>

#include "slg_collapse.hpp"

using namespace slghost;

static_assert(slg::kCollapseMaxRows == SLG_MAX_COLLAPSE_ROWS, "the kernel's LDS rows and the ABI's limit on k");
static_assert(slg::kCollapseSortParts == SLG_MAX_SORT_PARTS, "the inner sort's parts");
static_assert(SLG_MAX_INNER_HITS == 64u, "one kept member per lane of a wave");

namespace {
// the words of side array i of a batch (slg::collapse_side: the layout the kernel writes)
size_t side_off(const slg_batch *b, uint32_t i) { return slg::collapse_side(i, b->nq, b->cl_groups, b->cl_size); }
}  // namespace

void slghost::collapse_attach(slg_batch *b, const slg_collapse_spec &spec, const slg_sort_spec *batch_sort) {
  const IndexState &S = *b->snap;
  slg_index *ix = b->idx;
  const size_t n_segs = S.segs.size();
  const auto it = S.agg_fields.find(spec.field);
  SLG_REQUIRE(it != S.agg_fields.end(), "collapse: unknown agg field id " + std::to_string(spec.field));
  const AggFieldData &fd = *it->second;
  SLG_REQUIRE(fd.kind == 2, "collapse: field " + std::to_string(spec.field) + " is a numeric field (keyword columns only)");
  std::vector<slg::CollapseColDev> cols(std::max<size_t>(n_segs, 1), slg::CollapseColDev{nullptr, nullptr});
  for (size_t s = 0; s < n_segs; s++) {
    SLG_REQUIRE(s < fd.per_seg.size() && fd.per_seg[s],
                "collapse: agg field " + std::to_string(spec.field) + " has no column for segment " + std::to_string(s) +
                    " (added after the field was registered)");
    const AggColumn &c = *fd.per_seg[s];
    cols[s] = slg::CollapseColDev{c.offs.as<const uint32_t>(), c.vals.as<const uint32_t>()};
  }
  // the inner sort: none, or one that equals the batch's own order (score order: `_score` desc), leaves the
  // members in row order; an empty one is `_score` desc (query/sort.rs:159-167)
  slg_sort_spec inner{}, own{};
  own.n_parts = 1;
  own.field[0] = SLG_SORT_SCORE;
  own.order[0] = SLG_ORDER_DESC;
  if (batch_sort) own = *batch_sort;
  bool resort = spec.inner_sort != nullptr && spec.inner_size > 0;
  if (resort) {
    inner = spec.inner_sort->n_parts ? *spec.inner_sort : slg_sort_spec{1, {SLG_SORT_SCORE}, {SLG_ORDER_DESC}};
    bool same = inner.n_parts == own.n_parts;
    for (uint32_t i = 0; same && i < inner.n_parts; i++)
      same = inner.field[i] == own.field[i] && inner.order[i] == own.order[i];
    resort = !same;
  }
  std::vector<slg::CollapseSortColDev> scols(slg::kCollapseSortParts * std::max<size_t>(n_segs, 1),
                                             slg::CollapseSortColDev{nullptr, nullptr});
  b->cl_parts = b->cl_score_parts = b->cl_desc_parts = 0;
  for (uint32_t i = 0; resort && i < inner.n_parts; i++) {
    if (inner.order[i] == SLG_ORDER_DESC) b->cl_desc_parts |= 1u << i;
    if (inner.field[i] == SLG_SORT_SCORE) {
      b->cl_score_parts |= 1u << i;
      continue;
    }
    const auto sf = S.sort_fields.find(inner.field[i]);
    SLG_REQUIRE(sf != S.sort_fields.end(), "collapse: unknown sort field id in inner sort part " + std::to_string(i));
    for (size_t s = 0; s < n_segs; s++) {
      SLG_REQUIRE(s < sf->second->per_seg.size() && sf->second->per_seg[s],
                  "collapse: sort field " + std::to_string(inner.field[i]) + " has no column for segment " +
                      std::to_string(s) + " (added after the field was registered)");
      const SortColumn &c = *sf->second->per_seg[s];
      scols[i * n_segs + s] = slg::CollapseSortColDev{c.key[inner.order[i]].as<const unsigned long long>(),
                                                      c.present.as<const uint32_t>()};
    }
  }
  if (resort) b->cl_parts = inner.n_parts;
  b->collapse = true;
  b->cl_groups = spec.group_limit;
  b->cl_from = spec.inner_from;
  b->cl_size = spec.inner_size;
  b->cl_lds_rows = slg::collapse_lds_rows(b->k);
  upload_image(b->d_cl_desc, &ix->pool, {image_part(cols), image_part(scols)});
  b->d_cl_side.alloc_pooled(&ix->pool, (side_off(b, slg::kClArrays) + 1) * 4);  // (+ the error word)
}

void slghost::collapse_launch(slg_batch *b, hipStream_t st) {
  if (b->nq == 0) return;
  const IndexState &S = *b->snap;
  const size_t n_segs = S.segs.size();
  slg::CollapseParams p{};
  p.cols = b->d_cl_desc.as<const slg::CollapseColDev>();
  p.scols = reinterpret_cast<const slg::CollapseSortColDev *>(p.cols + std::max<size_t>(n_segs, 1));
  p.n_segs = (uint32_t)n_segs;
  p.n_parts = b->cl_parts;
  p.score_parts = b->cl_score_parts;
  p.desc_parts = b->cl_desc_parts;
  p.out_doc = b->d_out_doc;
  p.out_seg = b->d_out_seg;
  p.out_score = b->d_out_score;
  p.out_count = b->d_out_count;
  p.nq = b->nq;
  p.k = b->k;
  p.groups = b->cl_groups;
  p.from = b->cl_from;
  p.size = b->cl_size;
  p.lds_rows = b->cl_lds_rows;
  p.side = b->d_cl_side.as<uint32_t>();
  p.flag = ResultBlock(b->nq, b->k).flag(b->d_out.as<uint32_t>());
  SLG_HIP(slg::launch_with_lds(slg::collapse_kernel, p, p.nq, slg::collapse_lds_bytes(p.lds_rows), st));
}

extern "C" {

int slg_batch_fetch_collapse(slg_batch *b, uint32_t *n_groups, uint32_t *total_groups, uint32_t *status,
                             uint32_t *group_row, uint32_t *group_ord, uint32_t *group_size, uint32_t *group_doc,
                             uint32_t *group_seg, float *group_score, uint32_t *inner_count, uint32_t *inner_row,
                             uint32_t *inner_doc, uint32_t *inner_seg, float *inner_score) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->collapse, "not a collapse batch (slg_batch_prepare_collapse)");
    SLG_REQUIRE(b->launched, "the batch has not run");
    DeviceGuard g(b->idx->device);
    const hipStream_t st = locked_stream(b);
    if (b->nq == 0) return;
    // the arrays and the error word behind them are one block: ONE D2H copy, small blocks into pageable memory,
    // large ones into a pinned image of the index's pool (as slg_batch_fetch)
    const size_t words = side_off(b, slg::kClArrays) + 1;
    std::optional<ImageLease> lease;
    std::vector<uint32_t> pageable;
    uint32_t *blk = nullptr;
    if (words * 4 <= (256u << 10)) {
      pageable.resize(words);
      blk = pageable.data();
    } else {
      lease.emplace(b->idx->pool, words * 4);
      blk = static_cast<uint32_t *>(lease->p);
    }
    SLG_HIP(hipMemcpyAsync(blk, b->d_cl_side.p, words * 4, hipMemcpyDeviceToHost, st));
    SLG_HIP(wait_stream(st));
    if (blk[words - 1] != 0u)  // rows a scoring wave gave up on are not collapsed into an answer
      throw SlgError(SLG_ERR_INTERNAL, "a scoring wave gave up on a round (chunk-loop guard): results are incomplete");
    void *const dst[14] = {n_groups,  total_groups, status,      group_row, group_ord, group_size, group_doc,
                           group_seg, group_score,  inner_count, inner_row, inner_doc, inner_seg,  inner_score};
    for (uint32_t i = 0; i < slg::kClArrays; i++) {
      const size_t n = side_off(b, i + 1) - side_off(b, i);
      if (dst[i] && n) std::memcpy(dst[i], blk + side_off(b, i), n * 4);
    }
  });
}

}  // extern "C"
