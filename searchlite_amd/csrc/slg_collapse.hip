// slg_collapse.hip — collapse batches (slg_batch_prepare_collapse): the spec against the batch's index state,
// the column tables and side arrays on the device, the launch of collapse_kernel behind the batch's rows, and
// slg_batch_fetch_collapse.  (The checks of a spec that need no index: slg_plan.cpp, check_collapse.)
#include "slg_host.hpp"

#include "slg_collapse.hpp"

using namespace slghost;

static_assert(slg::kCollapseMaxRows == SLG_MAX_COLLAPSE_ROWS, "the kernel's LDS rows and the ABI's limit on k");
static_assert(slg::kSortMaxParts == SLG_MAX_SORT_PARTS, "the inner sort's parts");
static_assert(SLG_MAX_INNER_HITS == 64u, "one kept member per lane of a wave");

namespace {
// the words of side array i of a batch (slg::collapse_side: the layout the kernel writes)
size_t side_off(const slg_batch *b, uint32_t i) { return slg::collapse_side(i, b->nq, b->cl_groups, b->cl_size); }
}  // namespace

void slghost::collapse_attach(slg_batch *b, const slg_collapse_spec &spec, const slg_sort_spec *batch_sort) {
  const IndexState &S = *b->snap;
  slg_index *ix = b->idx;
  const size_t n_segs = S.segs.size();
  const std::vector<slgplan::FscoreFieldView> fields = fscore_field_views(S);
  const slgplan::FscoreFieldView &fd = slgplan::agg_field(fields, spec.field, "collapse: ", "");
  SLG_REQUIRE(fd.keyword, "collapse: field " + std::to_string(spec.field) + " is a numeric field (keyword columns only)");
  std::vector<slg::ColumnDev> cols(std::max<size_t>(n_segs, 1), slg::ColumnDev{nullptr, nullptr});
  std::copy_n(slgplan::agg_field_rows(fd, (uint32_t)n_segs, "collapse: ", ""), n_segs, cols.begin());
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
  if (!resort) inner = slg_sort_spec{};  // (no part: an all-null table, the members stay in row order)
  const SortBinding sorting = bind_sort(S, inner, "collapse: ", "inner sort part ");
  b->cl_parts = inner.n_parts;
  b->cl_score_parts = sorting.score_parts;
  b->cl_desc_parts = sorting.desc_parts;
  b->collapse = true;
  b->cl_groups = spec.group_limit;
  b->cl_from = spec.inner_from;
  b->cl_size = spec.inner_size;
  b->cl_lds_rows = slg::collapse_lds_rows(b->k);
  upload_image(b->d_cl_desc, &ix->pool, {image_part(cols), image_part(sorting.cols)});
  b->d_cl_side.alloc_pooled(&ix->pool, (side_off(b, slg::kClArrays) + 1) * 4);  // (+ the error word)
}

void slghost::collapse_launch(slg_batch *b, hipStream_t st) {
  if (b->nq == 0) return;
  const IndexState &S = *b->snap;
  const size_t n_segs = S.segs.size();
  slg::CollapseParams p{};
  p.cols = b->d_cl_desc.as<const slg::ColumnDev>();
  p.sort_cols = reinterpret_cast<const slg::SortColDev *>(p.cols + std::max<size_t>(n_segs, 1));
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
    // the arrays and the error word behind them are one block
    const size_t words = side_off(b, slg::kClArrays) + 1;
    const SideBlock host(b, b->d_cl_side, words, st);
    const uint32_t *const blk = host.p;
    void *const dst[14] = {n_groups,  total_groups, status,      group_row, group_ord, group_size, group_doc,
                           group_seg, group_score,  inner_count, inner_row, inner_doc, inner_seg,  inner_score};
    for (uint32_t i = 0; i < slg::kClArrays; i++) {
      const size_t n = side_off(b, i + 1) - side_off(b, i);
      if (dst[i] && n) std::memcpy(dst[i], blk + side_off(b, i), n * 4);
    }
  });
}

}  // extern "C"
