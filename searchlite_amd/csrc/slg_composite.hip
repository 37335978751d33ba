// slg_composite.hip — composite batches (slg_batch_prepare_composite): the checks of a spec, the packed key layout
// against the batch's index state, the children's tables (planned by slg_aggs.hip as the roots of `size` parent
// rows), descriptors, ranks, bounds and tables on the device, the launches of composite_select_kernel and
// composite_collect_kernel behind agg_kernel, and slg_batch_composite_layout / _set_composite_after /
// _fetch_composite.
#include "slg_host.hpp"

#include <cmath>

#include "slg_composite.hpp"

using namespace slghost;

static_assert(slg::kCpMaxSources == SLG_MAX_COMPOSITE_SOURCES && slg::kCpMaxSize == SLG_MAX_COMPOSITE_SIZE,
              "the kernel's limits and the ABI's");
static_assert(slg::kCpTerms == SLG_COMPOSITE_TERMS && slg::kCpHistogram == SLG_COMPOSITE_HISTOGRAM, "source kinds");
static_assert(sizeof(slg::CompositeSourceDev) % 8 == 0 && sizeof(slg::AggNodeDev) % 8 == 0, "records of whole words");

namespace {
std::string source_name(uint32_t i) { return "composite source " + std::to_string(i); }
uint32_t ceil_log2_64(uint64_t n) {
  uint32_t l = 0;
  while (l < 63 && (1ull << l) < n) l++;
  return l;
}
bool is_value_kind(int32_t kind) {
  return kind == SLG_AGG_CARDINALITY || kind == SLG_AGG_PERCENTILES || kind == SLG_AGG_PERCENTILE_RANKS;
}
// the words of d_cp_out: the keys, n_buckets, has_more, the error word
size_t out_words(const slg_batch *b) {
  const size_t nq = std::max<uint32_t>(b->nq, 1);
  return 2 * nq * b->cp_spec.size + 2 * nq + 1;
}
}  // namespace

void slghost::composite_check_spec(const slg_composite_spec *spec) {
  SLG_REQUIRE(spec != nullptr, "composite spec is NULL");
  SLG_REQUIRE(spec->n_sources >= 1, "a composite spec needs at least one source");
  const uint32_t ns = std::min<uint32_t>(spec->n_sources, SLG_MAX_COMPOSITE_SOURCES);
  for (uint32_t i = 0; i < ns; i++) {
    const slg_composite_source &s = spec->sources[i];
    SLG_REQUIRE(s.kind == SLG_COMPOSITE_TERMS || s.kind == SLG_COMPOSITE_HISTOGRAM, source_name(i) + ": unknown kind");
    if (s.kind == SLG_COMPOSITE_HISTOGRAM)
      SLG_REQUIRE(std::isfinite(s.interval) && s.interval > 0.0,
                  source_name(i) + ": interval must be positive and finite");
  }
  // the children as slg_batch_prepare_aggs would see them as roots (an invalid child is reported before anything
  // unsupported; a child kind that is known but not built under a composite comes after)
  const uint32_t nc = std::min<uint32_t>(spec->n_children, SLG_MAX_AGGS);
  std::string unsupported;
  if (nc) {
    slg_agg_spec roots{};
    roots.n_nodes = nc;
    for (uint32_t i = 0; i < nc; i++) {
      roots.nodes[i] = spec->children[i];
      roots.nodes[i].parent = -1;
    }
    try {
      agg_check_spec(&roots);
    } catch (const SlgError &e) {
      if (e.code != SLG_ERR_UNSUPPORTED) throw SlgError(e.code, std::string("composite child: ") + e.what());
      unsupported = std::string("composite child: ") + e.what();
    }
  }
  if (spec->n_sources > SLG_MAX_COMPOSITE_SOURCES)
    throw SlgError(SLG_ERR_UNSUPPORTED, "more than SLG_MAX_COMPOSITE_SOURCES composite sources");
  if (spec->size == 0) throw SlgError(SLG_ERR_UNSUPPORTED, "composite size is 0 (the response is empty: CPU path)");
  if (spec->size > SLG_MAX_COMPOSITE_SIZE) throw SlgError(SLG_ERR_UNSUPPORTED, "composite size > SLG_MAX_COMPOSITE_SIZE");
  if (spec->n_children > SLG_MAX_AGGS) throw SlgError(SLG_ERR_UNSUPPORTED, "more than SLG_MAX_AGGS composite children");
  if (!unsupported.empty()) throw SlgError(SLG_ERR_UNSUPPORTED, unsupported);
  for (uint32_t i = 0; i < nc; i++)
    if (is_value_kind(spec->children[i].kind))
      throw SlgError(SLG_ERR_UNSUPPORTED, "composite child " + std::to_string(i) +
                                              ": cardinality, percentiles and percentile_ranks are not built under a "
                                              "composite (CPU path)");
}

void slghost::composite_attach(slg_batch *b, const slg_composite_spec &spec) {
  const IndexState &S = *b->snap;
  slg_index *ix = b->idx;
  const size_t n_segs = S.segs.size();
  const uint32_t ns = spec.n_sources;
  const std::vector<slgplan::FscoreFieldView> fields = fscore_field_views(S);
  std::vector<slg::CompositeSourceDev> src(ns);
  std::vector<slg::ColumnDev> src_cols((size_t)ns * std::max<size_t>(n_segs, 1), slg::ColumnDev{nullptr, nullptr});
  std::vector<uint32_t> ranks;           // the ord_rank of every terms source that has one, back to back
  std::vector<size_t> rank_at(ns, ~(size_t)0);
  std::vector<const slgplan::FscoreFieldView *> fds(ns, nullptr);
  for (uint32_t i = 0; i < ns; i++) {  // what is invalid, for every source, before what is unsupported
    const slg_composite_source &s = spec.sources[i];
    const bool terms = s.kind == SLG_COMPOSITE_TERMS;
    const slgplan::FscoreFieldView &fd = slgplan::agg_field(fields, s.field, source_name(i) + ": ", "");
    fds[i] = &fd;
    std::copy_n(slgplan::agg_field_rows(fd, (uint32_t)n_segs, source_name(i) + ": ", ""), n_segs,
                src_cols.begin() + (size_t)i * n_segs);
    SLG_REQUIRE(terms == fd.keyword, source_name(i) + ": field " + std::to_string(s.field) +
                                         (fd.keyword ? " is a keyword field (a terms source only)"
                                                     : " is a numeric field (a histogram source only)"));
    if (terms && s.ord_rank) {
      std::vector<char> seen(fd.n_ords, 0);
      for (uint32_t o = 0; o < fd.n_ords; o++) {
        const uint32_t r = s.ord_rank[o];
        SLG_REQUIRE(r < fd.n_ords && !seen[r], source_name(i) + ": ord_rank is not a permutation of [0, n_ords)");
        seen[r] = 1;
      }
      rank_at[i] = ranks.size();
      ranks.insert(ranks.end(), s.ord_rank, s.ord_rank + fd.n_ords);
    }
  }
  slg_composite_layout lay{};
  lay.n_sources = ns;
  lay.size = spec.size;
  lay.n_children = spec.n_children;
  uint32_t key_bits = 0;
  for (uint32_t i = 0; i < ns; i++) {
    const slg_composite_source &s = spec.sources[i];
    const slgplan::FscoreFieldView &fd = *fds[i];
    slg_composite_source_layout &L = lay.sources[i];
    L.first_id = 0;
    L.zero_slot = -1;
    if (s.kind == SLG_COMPOSITE_TERMS) {
      L.slots = std::max<uint64_t>(fd.n_ords, 1);
    } else {
      if (fd.non_finite)
        throw SlgError(SLG_ERR_UNSUPPORTED, source_name(i) + ": agg field " + std::to_string(s.field) +
                                                " holds a non-finite value (CPU path)");
      if (fd.from_i64)  // (f64_values sees f64 columns only: the reference skips every doc)
        throw SlgError(SLG_ERR_UNSUPPORTED, source_name(i) + ": agg field " + std::to_string(s.field) +
                                                " was registered from i64 values (the response is empty: CPU path)");
      L.slots = 1;  // (a column without a value: one slot, never emitted)
      if (fd.any_value) {
        // the id range: floor(v / interval) is monotone in v (this unit is compiled without fast-math, as the kernel)
        const double klo = std::floor(fd.vmin / s.interval), khi = std::floor(fd.vmax / s.interval);
        if (!(std::fabs(klo) < 2147483648.0 && std::fabs(khi) < 2147483648.0))
          throw SlgError(SLG_ERR_UNSUPPORTED, source_name(i) + ": a histogram id at or beyond +-2^31 (CPU path)");
        L.first_id = (int64_t)klo;
        const int64_t last = (int64_t)khi;
        const bool zero = L.first_id <= 0 && last >= 0;
        L.zero_slot = zero ? -L.first_id : -1;
        L.slots = (uint64_t)(last - L.first_id + 1) + (zero ? 1u : 0u);
      }
    }
    L.bits = ceil_log2_64(L.slots);
    key_bits += L.bits;
  }
  if (key_bits > 63) throw SlgError(SLG_ERR_UNSUPPORTED, "a composite key of more than 63 bits (CPU path)");
  lay.key_bits = key_bits;
  for (uint32_t i = 0, below = key_bits; i < ns; i++) {
    below -= lay.sources[i].bits;
    lay.sources[i].shift = below;
  }
  // the tables: behind the cells of the aggregation spec in a query's rows; `size` count cells, then the children
  const AggSpecCells spec_cells = agg_spec_cells(b);
  const uint64_t agg_cells = spec_cells.all();
  if (agg_cells + spec.size > SLG_MAX_AGG_CELLS)
    throw SlgError(SLG_ERR_UNSUPPORTED, "more than SLG_MAX_AGG_CELLS aggregation cells per query (at the composite)");
  const CompositeChildTables ch = agg_plan_children(S, spec, agg_cells);
  const uint32_t ac = spec_cells.count, as = spec_cells.stats;
  lay.count_offset = ac;
  for (uint32_t i = 0; i < spec.n_children; i++) {
    lay.children[i] = ch.layout[i];
    lay.children[i].offset += lay.children[i].is_stats ? as : ac;
  }
  b->composite = true;
  b->cp_spec = spec;
  for (uint32_t i = 0; i < SLG_MAX_COMPOSITE_SOURCES; i++) b->cp_spec.sources[i].ord_rank = nullptr;
  b->cp_layout = lay;
  b->cp_count_cells = (uint32_t)ch.count_cells;
  b->cp_stats_cells = (uint32_t)ch.stats_cells;
  b->cp_cap = slg::cp_cap(spec.size);
  b->cp_lds = 4 * ch.count_cells + sizeof(slg::AggStatDev) * ch.stats_cells <= slg::kAggLdsBytes;
  b->cp_ext = ch.ext;

  if (!ranks.empty()) {
    b->d_cp_ranks.alloc_pooled(&ix->pool, ranks.size() * 4);
    SLG_HIP(hipMemcpy(b->d_cp_ranks.p, ranks.data(), ranks.size() * 4, hipMemcpyHostToDevice));
  }
  for (uint32_t i = 0; i < ns; i++) {
    const slg_composite_source_layout &L = lay.sources[i];
    slg::CompositeSourceDev &d = src[i];
    d = slg::CompositeSourceDev{};
    d.kind = spec.sources[i].kind;
    d.shift = L.shift;
    d.n_ords = fds[i]->n_ords;
    d.ord_rank = rank_at[i] == ~(size_t)0 ? nullptr : b->d_cp_ranks.as<const uint32_t>() + rank_at[i];
    d.interval = spec.sources[i].interval;
    d.first_id = L.first_id;
    d.zero_slot = L.zero_slot;
    d.slots = L.slots;
  }
  b->cp_cols_off = ch.nodes.size();
  b->cp_src_cols_off = b->cp_cols_off + ch.cols.size();
  b->cp_src_off = b->cp_src_cols_off + src_cols.size() * sizeof(slg::ColumnDev);
  upload_image(b->d_cp_desc, &ix->pool,
               {ImagePart{ch.nodes.data(), ch.nodes.size()}, ImagePart{ch.cols.data(), ch.cols.size()},
                image_part(src_cols), image_part(src)});
  const size_t nq = std::max<uint32_t>(b->nq, 1);
  b->d_cp_lower.alloc_pooled(&ix->pool, nq * 8);
  SLG_HIP(hipMemset(b->d_cp_lower.p, 0, nq * 8));
  b->d_cp_out.alloc_pooled(&ix->pool, out_words(b) * 4);
  b->d_cp_counts.alloc_pooled(&ix->pool, nq * std::max<size_t>(b->cp_count_cells, 1) * 4);
  b->d_cp_stats.alloc_pooled(&ix->pool, nq * std::max<size_t>(b->cp_stats_cells, 1) * sizeof(slg::AggStatDev));
}

void slghost::composite_launch(slg_batch *b, hipStream_t st) {
  if (b->nq == 0) return;
  const size_t nq = b->nq;
  slg::CompositeParams p{};
  fill_candidates(p.a, b);
  unsigned char *const desc = b->d_cp_desc.as<unsigned char>();
  p.a.nodes = reinterpret_cast<const slg::AggNodeDev *>(desc);
  p.a.cols = reinterpret_cast<const slg::ColumnDev *>(desc + b->cp_cols_off);
  p.a.n_nodes = b->cp_spec.n_children;
  p.a.nq = b->nq;
  p.a.count_cells = b->cp_count_cells;
  p.a.stats_cells = b->cp_stats_cells;
  p.a.counts = b->d_cp_counts.as<uint32_t>();
  p.a.stats = b->d_cp_stats.as<slg::AggStatDev>();
  // a sorted batch's select counted the accepted docs, agg_kernel does in score order; without either the collect
  p.a.out_matched = post_select_matched(b);
  p.src_cols = reinterpret_cast<const slg::ColumnDev *>(desc + b->cp_src_cols_off);
  p.src = reinterpret_cast<const slg::CompositeSourceDev *>(desc + b->cp_src_off);
  p.n_sources = b->cp_spec.n_sources;
  p.size = b->cp_spec.size;
  p.cap = b->cp_cap;
  p.q_lower = b->d_cp_lower.as<const unsigned long long>();
  p.keys = b->d_cp_out.as<unsigned long long>();
  p.n_buckets = b->d_cp_out.as<uint32_t>() + 2 * nq * p.size;
  p.has_more = p.n_buckets + nq;
  p.err = p.has_more + nq;
  p.flag = ResultBlock(b->nq, b->k).flag(b->d_out.as<uint32_t>());
  launch_kernel_lds(slg::composite_select_kernel, p, dim3(b->nq), slg::kCpThreads,
                    (size_t)slg::kCpWaves * p.cap * 8, st);
  const size_t keys_lds = (size_t)p.size * 8;
  if (b->cp_lds) {
    const size_t lds = keys_lds + (size_t)p.a.stats_cells * sizeof(slg::AggStatDev) + (size_t)p.a.count_cells * 4;
    launch_kernel_lds(b->cp_ext ? slg::composite_collect_kernel<true, true> : slg::composite_collect_kernel<true, false>,
                      p, dim3(b->nq), slg::kCpThreads, lds, st);
  } else {
    SLG_HIP(hipMemsetAsync(b->d_cp_counts.p, 0, nq * std::max<size_t>(p.a.count_cells, 1) * 4, st));
    SLG_HIP(hipMemsetAsync(b->d_cp_stats.p, 0, nq * std::max<size_t>(p.a.stats_cells, 1) * sizeof(slg::AggStatDev), st));
    launch_kernel_lds(b->cp_ext ? slg::composite_collect_kernel<false, true> : slg::composite_collect_kernel<false, false>,
                      p, dim3(b->nq), slg::kCpThreads, keys_lds, st);
  }
}

extern "C" {

int slg_batch_composite_layout(const slg_batch *b, slg_composite_layout *out) {
  return guarded([&] {
    SLG_REQUIRE(b != nullptr, "batch is NULL");
    SLG_REQUIRE(b->composite, "not a composite batch (slg_batch_prepare_composite)");
    SLG_REQUIRE(out != nullptr, "out is NULL");
    *out = b->cp_layout;
  });
}

int slg_batch_set_composite_after(slg_batch *b, const uint64_t *q_lower) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->composite, "not a composite batch (slg_batch_prepare_composite)");
    if (b->nq == 0) return;
    DeviceGuard g(b->idx->device);
    const hipStream_t st = locked_stream(b);
    // (behind the batch's last run on its stream; the copy of pageable memory has left the caller's array on return)
    if (q_lower) SLG_HIP(hipMemcpyAsync(b->d_cp_lower.p, q_lower, (size_t)b->nq * 8, hipMemcpyHostToDevice, st));
    else SLG_HIP(hipMemsetAsync(b->d_cp_lower.p, 0, (size_t)b->nq * 8, st));
    SLG_HIP(wait_stream(st));
  });
}

int slg_batch_fetch_composite(slg_batch *b, uint64_t *keys, uint32_t *n_buckets, uint32_t *has_more) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->composite, "not a composite batch (slg_batch_prepare_composite)");
    SLG_REQUIRE(b->launched, "the batch has not run");
    DeviceGuard g(b->idx->device);
    const hipStream_t st = locked_stream(b);
    if (b->nq == 0) return;
    // the arrays and the error word behind them are one block
    const size_t words = out_words(b), nq = b->nq, kw = 2 * nq * b->cp_spec.size;
    const SideBlock host(b, b->d_cp_out, words, st);
    const uint32_t *const blk = host.p;
    if (keys) std::memcpy(keys, blk, kw * 4);
    if (n_buckets) std::memcpy(n_buckets, blk + kw, nq * 4);
    if (has_more) std::memcpy(has_more, blk + kw + nq, nq * 4);
  });
}

}  // extern "C"
