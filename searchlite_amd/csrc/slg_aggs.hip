// slg_aggs.hip — aggregation batches (slg_batch_prepare_aggs): the checks of a spec, the layout of its
// tables, the launch of agg_kernel behind the batch's select kernel, and slg_batch_agg_layout / _fetch_aggs.
#include "slg_host.hpp"

#include <cmath>

#include "slg_aggs.hpp"

using namespace slghost;

static_assert(slg::kAggLdsBytes == SLG_AGG_LDS_BYTES && slg::kAggMaxRanges == SLG_MAX_AGG_RANGES, "header constants");
static_assert(slg::kAggTerms == SLG_AGG_TERMS && slg::kAggHistogram == SLG_AGG_HISTOGRAM &&
                  slg::kAggRange == SLG_AGG_RANGE && slg::kAggStats == SLG_AGG_STATS, "header kinds");
static_assert(sizeof(slg::AggStatDev) == 32 && sizeof(slg_agg_stats) == 32, "stats cells are 32 bytes");

namespace {
bool is_bucket(int32_t kind) { return kind == SLG_AGG_TERMS || kind == SLG_AGG_HISTOGRAM || kind == SLG_AGG_RANGE; }
std::string node_name(uint32_t i) { return "agg node " + std::to_string(i); }

// floor((val - offset) / interval), the reference's bucket_key (aggs/mod.rs:1162-1164) in IEEE f64 (host
// code of this unit is compiled without fast-math and without contraction, as the kernel)
double bucket_key(double val, double offset, double interval) { return std::floor((val - offset) / interval); }
}  // namespace

void slghost::agg_check_spec(const slg_agg_spec *aggs) {
  SLG_REQUIRE(aggs != nullptr, "aggs is NULL");
  SLG_REQUIRE(aggs->n_nodes >= 1, "an aggregation spec needs at least one node");
  if (aggs->n_nodes > SLG_MAX_AGGS) throw SlgError(SLG_ERR_UNSUPPORTED, "more than SLG_MAX_AGGS aggregation nodes");
  for (uint32_t i = 0; i < aggs->n_nodes; i++) {
    const slg_agg_node &n = aggs->nodes[i];
    SLG_REQUIRE(n.kind == SLG_AGG_STATS || is_bucket(n.kind), node_name(i) + ": unknown kind");
    if (n.parent != -1) {
      SLG_REQUIRE(n.parent >= 0 && (uint32_t)n.parent < i, node_name(i) + ": parent is not an earlier node");
      const slg_agg_node &pn = aggs->nodes[n.parent];
      SLG_REQUIRE(is_bucket(pn.kind), node_name(i) + ": parent is not a bucket node (terms, histogram, range)");
      SLG_REQUIRE(pn.parent == -1, node_name(i) + ": parent is not a root (two levels)");
    }
    if (n.kind != SLG_AGG_TERMS && n.has_missing)
      SLG_REQUIRE(std::isfinite(n.missing), node_name(i) + ": missing is not finite");
    if (n.kind == SLG_AGG_HISTOGRAM) {
      SLG_REQUIRE(std::isfinite(n.interval) && n.interval > 0.0, node_name(i) + ": interval must be positive and finite");
      SLG_REQUIRE(std::isfinite(n.offset), node_name(i) + ": offset is not finite");
      if (n.has_hard_bounds)
        SLG_REQUIRE(!std::isnan(n.hard_min) && !std::isnan(n.hard_max), node_name(i) + ": hard bound is NaN");
    }
    if (n.kind == SLG_AGG_RANGE) {
      SLG_REQUIRE(n.n_ranges >= 1, node_name(i) + ": a range node needs at least one range");
      if (n.n_ranges > SLG_MAX_AGG_RANGES)
        throw SlgError(SLG_ERR_UNSUPPORTED, node_name(i) + ": more than SLG_MAX_AGG_RANGES ranges");
      for (uint32_t r = 0; r < n.n_ranges; r++)
        SLG_REQUIRE(!std::isnan(n.from[r]) && !std::isnan(n.to[r]), node_name(i) + ": range bound is NaN");
    }
  }
}

// The spec against the batch's index state: fields, the tables' layout, the device descriptors and tables
void slghost::agg_attach(slg_batch *b, const slg_agg_spec &aggs) {
  const IndexState &S = *b->snap;
  slg_index *ix = b->idx;
  const size_t n_segs = S.segs.size();
  const uint32_t nn = aggs.n_nodes;
  std::vector<slg::AggNodeDev> nodes(nn);
  std::vector<slg::ColumnDev> cols((size_t)nn * std::max<size_t>(n_segs, 1), slg::ColumnDev{nullptr, nullptr});
  const std::vector<slgplan::FscoreFieldView> fields = fscore_field_views(S);
  b->agg_layout.assign(nn, slg_agg_layout{});
  uint64_t count_cells = 0, stats_cells = 0;
  for (uint32_t i = 0; i < nn; i++) {
    const slg_agg_node &n = aggs.nodes[i];
    const slgplan::FscoreFieldView &fd = slgplan::agg_field(fields, n.field, node_name(i) + ": ", "");
    SLG_REQUIRE((n.kind == SLG_AGG_TERMS) == fd.keyword,
                node_name(i) + ": field " + std::to_string(n.field) +
                    (fd.keyword ? " is a keyword field (terms only)" : " is a numeric field (not for terms)"));
    std::copy_n(slgplan::agg_field_rows(fd, (uint32_t)n_segs, "", ""), n_segs, cols.begin() + (size_t)i * n_segs);
    if (!fd.keyword && fd.non_finite)
      throw SlgError(SLG_ERR_UNSUPPORTED,
                     node_name(i) + ": agg field " + std::to_string(n.field) + " holds a non-finite value (CPU path)");
    slg::AggNodeDev &d = nodes[i];
    d = slg::AggNodeDev{};
    d.kind = n.kind;
    d.parent = n.parent;
    d.col = i;
    d.has_missing = n.has_missing ? 1u : 0u;
    d.missing = n.missing;
    uint64_t rows = 1;
    long long first_id = 0;
    if (n.kind == SLG_AGG_TERMS) {
      if (n.has_missing) SLG_REQUIRE(n.missing_ord <= fd.n_ords, node_name(i) + ": missing_ord > n_ords");
      d.n_ords = fd.n_ords;
      d.missing_ord = n.missing_ord;
      rows = (uint64_t)fd.n_ords + ((n.has_missing && n.missing_ord == fd.n_ords) ? 1u : 0u);
    } else if (n.kind == SLG_AGG_HISTOGRAM) {
      d.interval = n.interval;
      d.offset = n.offset;
      d.has_hard = n.has_hard_bounds ? 1u : 0u;
      d.hard_min = n.hard_min;
      d.hard_max = n.hard_max;
      // the dense id range: the bucket formula is monotone in val, so the ids of the smallest and the largest
      // value that can be collected bound every id (values outside the hard bounds are never collected)
      bool any = fd.any_value;
      double lo = fd.vmin, hi = fd.vmax;
      if (n.has_missing) {
        lo = any ? std::min(lo, n.missing) : n.missing;
        hi = any ? std::max(hi, n.missing) : n.missing;
        any = true;
      }
      if (any && n.has_hard_bounds) {
        lo = std::max(lo, n.hard_min);
        hi = std::min(hi, n.hard_max);
        any = lo <= hi;
      }
      if (any) {
        const double klo = bucket_key(lo, n.offset, n.interval), khi = bucket_key(hi, n.offset, n.interval);
        if (!(std::fabs(klo) < 9.0e15 && std::fabs(khi) < 9.0e15) || khi - klo + 1.0 > (double)SLG_MAX_AGG_CELLS)
          throw SlgError(SLG_ERR_UNSUPPORTED, node_name(i) + ": more than SLG_MAX_AGG_CELLS histogram buckets");
        first_id = (long long)klo;
        rows = (uint64_t)((long long)khi - first_id + 1);
      }
    } else if (n.kind == SLG_AGG_RANGE) {
      d.n_ranges = n.n_ranges;
      for (uint32_t r = 0; r < n.n_ranges; r++) {
        d.from[r] = n.from[r];
        d.to[r] = n.to[r];
      }
      rows = n.n_ranges;
    }
    if (rows == 0) rows = 1;  // (a keyword field without keys and without a missing row: one cell, never counted)
    const uint64_t parent_rows = n.parent < 0 ? 1u : b->agg_layout[n.parent].rows;
    uint64_t &cells = n.kind == SLG_AGG_STATS ? stats_cells : count_cells;
    if (rows > SLG_MAX_AGG_CELLS || parent_rows * rows > SLG_MAX_AGG_CELLS ||
        count_cells + stats_cells + parent_rows * rows > SLG_MAX_AGG_CELLS)
      throw SlgError(SLG_ERR_UNSUPPORTED, "more than SLG_MAX_AGG_CELLS aggregation cells per query (at " + node_name(i) + ")");
    d.rows = (uint32_t)rows;
    d.first_id = first_id;
    d.off = (uint32_t)cells;
    slg_agg_layout &lay = b->agg_layout[i];
    lay.parent_rows = (uint32_t)parent_rows;
    lay.rows = (uint32_t)rows;
    lay.first_id = first_id;
    lay.is_stats = n.kind == SLG_AGG_STATS ? 1u : 0u;
    lay.offset = cells;
    cells += parent_rows * rows;
  }
  b->aggs = true;
  b->agg_spec = aggs;
  b->agg_count_cells = (uint32_t)count_cells;
  b->agg_stats_cells = (uint32_t)stats_cells;
  b->agg_lds = 4 * count_cells + sizeof(slg::AggStatDev) * stats_cells <= slg::kAggLdsBytes;
  upload_image(b->d_agg_desc, &ix->pool, {image_part(nodes), image_part(cols)});
  const size_t nq = std::max<uint32_t>(b->nq, 1);
  b->d_agg_counts.alloc_pooled(&ix->pool, nq * std::max<size_t>(count_cells, 1) * 4);
  b->d_agg_stats.alloc_pooled(&ix->pool, nq * std::max<size_t>(stats_cells, 1) * sizeof(slg::AggStatDev));
}

void slghost::agg_launch(slg_batch *b, hipStream_t st) {
  if (b->nq == 0) return;
  slg::AggParams p{};
  fill_candidates(p, b);
  p.nodes = b->d_agg_desc.as<const slg::AggNodeDev>();
  p.cols = reinterpret_cast<const slg::ColumnDev *>(b->d_agg_desc.as<unsigned char>() +
                                                   (size_t)b->agg_spec.n_nodes * sizeof(slg::AggNodeDev));
  p.n_nodes = b->agg_spec.n_nodes;
  p.nq = b->nq;
  p.count_cells = b->agg_count_cells;
  p.stats_cells = b->agg_stats_cells;
  p.counts = b->d_agg_counts.as<uint32_t>();
  p.stats = b->d_agg_stats.as<slg::AggStatDev>();
  // a sorted batch's select counted the accepted docs; in score order this kernel does
  p.out_matched = b->sorted ? nullptr : b->d_matched.as<unsigned long long>();
  if (b->agg_lds) {
    const size_t lds = (size_t)p.stats_cells * sizeof(slg::AggStatDev) + (size_t)p.count_cells * 4;
    launch_kernel_lds(slg::agg_kernel<true>, p, dim3(b->nq), slg::kAggThreads, lds, st);
  } else {
    SLG_HIP(hipMemsetAsync(b->d_agg_counts.p, 0, (size_t)b->nq * std::max<size_t>(p.count_cells, 1) * 4, st));
    SLG_HIP(hipMemsetAsync(b->d_agg_stats.p, 0,
                           (size_t)b->nq * std::max<size_t>(p.stats_cells, 1) * sizeof(slg::AggStatDev), st));
    launch_kernel_lds(slg::agg_kernel<false>, p, dim3(b->nq), slg::kAggThreads, 0, st);
  }
}

extern "C" {

int slg_batch_agg_layout(const slg_batch *b, slg_agg_layout *out) {
  return guarded([&] {
    SLG_REQUIRE(b != nullptr, "batch is NULL");
    SLG_REQUIRE(b->aggs, "not an aggregation batch (slg_batch_prepare_aggs)");
    SLG_REQUIRE(out != nullptr, "out is NULL");
    std::copy(b->agg_layout.begin(), b->agg_layout.end(), out);
  });
}

int slg_batch_fetch_aggs(slg_batch *b, uint64_t *counts, slg_agg_stats *stats) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->aggs, "not an aggregation batch (slg_batch_prepare_aggs)");
    SLG_REQUIRE(b->launched, "the batch has not run");
    const size_t nc = (size_t)b->nq * b->agg_count_cells, ns = (size_t)b->nq * b->agg_stats_cells;
    SLG_REQUIRE(nc == 0 || counts != nullptr, "counts is NULL");
    SLG_REQUIRE(ns == 0 || stats != nullptr, "stats is NULL");
    DeviceGuard g(b->idx->device);
    const hipStream_t st = locked_stream(b);
    std::vector<uint32_t> hc(nc);
    std::vector<slg::AggStatDev> hs(ns);
    if (nc) SLG_HIP(hipMemcpyAsync(hc.data(), b->d_agg_counts.p, nc * 4, hipMemcpyDeviceToHost, st));
    if (ns) SLG_HIP(hipMemcpyAsync(hs.data(), b->d_agg_stats.p, ns * sizeof(slg::AggStatDev), hipMemcpyDeviceToHost, st));
    SLG_HIP(wait_stream(st));
    for (size_t i = 0; i < nc; i++) counts[i] = hc[i];
    auto value = [](unsigned long long key) {  // the inverse of agg_f64_key
      const unsigned long long bits = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
      double x;
      std::memcpy(&x, &bits, 8);
      return x;
    };
    for (size_t i = 0; i < ns; i++) {
      slg_agg_stats &o = stats[i];
      o = slg_agg_stats{0, 0.0, 0.0, 0.0};  // StatsState::default
      if (hs[i].count == 0) continue;
      o.count = hs[i].count;
      o.min = value(~hs[i].min_key);
      o.max = value(hs[i].max_key);
      o.sum = hs[i].sum;
    }
  });
}

}  // extern "C"
