// slg_aggs.hip — aggregation batches (slg_batch_prepare_aggs): the checks of a spec, the layout of its
// tables, the launch of agg_kernel (and, for a spec with value nodes, agg_values_kernel) behind the batch's select
// kernel, and slg_batch_agg_layout / _fetch_aggs / _fetch_agg_values.
#include "slg_host.hpp"

#include <cmath>

#include "slg_aggs.hpp"

using namespace slghost;

static_assert(slg::kAggLdsBytes == SLG_AGG_LDS_BYTES && slg::kAggMaxRanges == SLG_MAX_AGG_RANGES, "header constants");
static_assert(slg::kAggTerms == SLG_AGG_TERMS && slg::kAggHistogram == SLG_AGG_HISTOGRAM &&
                  slg::kAggRange == SLG_AGG_RANGE && slg::kAggStats == SLG_AGG_STATS, "header kinds");
static_assert(slg::kAggCardinality == SLG_AGG_CARDINALITY && slg::kAggPercentiles == SLG_AGG_PERCENTILES &&
                  slg::kAggPercentileRanks == SLG_AGG_PERCENTILE_RANKS && slg::kAggPctLdsBytes == SLG_AGG_PCT_LDS_BYTES,
              "header value kinds");
static_assert(slg::kAggDateHistogram == SLG_AGG_DATE_HISTOGRAM && slg::kAggFilter == SLG_AGG_FILTER &&
                  slg::kDateFixed == SLG_DATE_FIXED && slg::kDateDay == SLG_DATE_DAY && slg::kDateWeek == SLG_DATE_WEEK &&
                  slg::kDateMonth == SLG_DATE_MONTH && slg::kDateQuarter == SLG_DATE_QUARTER &&
                  slg::kDateYear == SLG_DATE_YEAR, "header date kinds");
static_assert(sizeof(slg::AggStatDev) == 32 && sizeof(slg_agg_stats) == 32, "stats cells are 32 bytes");

namespace {
bool is_bucket(int32_t kind) {
  return kind == SLG_AGG_TERMS || kind == SLG_AGG_HISTOGRAM || kind == SLG_AGG_RANGE ||
         kind == SLG_AGG_DATE_HISTOGRAM || kind == SLG_AGG_FILTER;
}
constexpr long long kTwo53 = 1ll << 53;  // an i64 up to here is an f64, and `as i64` / `as f64` are exact
bool within_two53(long long v) { return v >= -kTwo53 && v <= kTwo53; }
bool is_value(int32_t kind) {
  return kind == SLG_AGG_CARDINALITY || kind == SLG_AGG_PERCENTILES || kind == SLG_AGG_PERCENTILE_RANKS;
}
uint64_t f64_key(double x) {  // = slg::agg_f64_key
  uint64_t b;
  std::memcpy(&b, &x, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
uint32_t ceil_log2(uint32_t n) {
  uint32_t l = 0;
  while (l < 32 && (1ull << l) < n) l++;
  return l;
}
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
    SLG_REQUIRE(n.kind == SLG_AGG_STATS || is_bucket(n.kind) || is_value(n.kind), node_name(i) + ": unknown kind");
    if (n.parent != -1) {
      SLG_REQUIRE(n.parent >= 0 && (uint32_t)n.parent < i, node_name(i) + ": parent is not an earlier node");
      const slg_agg_node &pn = aggs->nodes[n.parent];
      SLG_REQUIRE(is_bucket(pn.kind), node_name(i) + ": parent is not a bucket node (terms, histogram, range, "
                                                     "date_histogram, filter)");
      SLG_REQUIRE(pn.parent == -1, node_name(i) + ": parent is not a root (two levels)");
    }
    // (a cardinality node's `missing` is read for a numeric field only: checked against the index)
    if (n.kind != SLG_AGG_TERMS && n.kind != SLG_AGG_CARDINALITY && n.kind != SLG_AGG_FILTER && n.has_missing)
      SLG_REQUIRE(std::isfinite(n.missing), node_name(i) + ": missing is not finite");
    if (n.kind == SLG_AGG_PERCENTILES || n.kind == SLG_AGG_PERCENTILE_RANKS) {
      const char *what = n.kind == SLG_AGG_PERCENTILES ? "percent" : "target";
      SLG_REQUIRE(n.n_ranges >= 1, node_name(i) + ": needs at least one " + what);
      if (n.n_ranges > SLG_MAX_AGG_RANGES)
        throw SlgError(SLG_ERR_UNSUPPORTED, node_name(i) + ": more than SLG_MAX_AGG_RANGES " + what + "s");
      for (uint32_t r = 0; r < n.n_ranges; r++)
        SLG_REQUIRE(!std::isnan(n.from[r]), node_name(i) + ": " + what + " is NaN");
      if (n.kind == SLG_AGG_PERCENTILES && n.parent != -1)
        throw SlgError(SLG_ERR_UNSUPPORTED, node_name(i) + ": a percentiles node is a root (not built as a child)");
    }
    if (n.kind == SLG_AGG_HISTOGRAM) {
      SLG_REQUIRE(std::isfinite(n.interval) && n.interval > 0.0, node_name(i) + ": interval must be positive and finite");
      SLG_REQUIRE(std::isfinite(n.offset), node_name(i) + ": offset is not finite");
      if (n.has_hard_bounds)
        SLG_REQUIRE(!std::isnan(n.hard_min) && !std::isnan(n.hard_max), node_name(i) + ": hard bound is NaN");
    }
    if (n.kind == SLG_AGG_FILTER) SLG_REQUIRE(n.filter >= 0, node_name(i) + ": filter id is negative");
    if (n.kind == SLG_AGG_DATE_HISTOGRAM) {
      SLG_REQUIRE(n.calendar_unit <= SLG_DATE_YEAR, node_name(i) + ": unknown calendar unit");
      if (n.calendar_unit == SLG_DATE_FIXED)
        SLG_REQUIRE(n.date_step >= 1, node_name(i) + ": a fixed interval must be at least 1 ms");
    }
    if (n.kind == SLG_AGG_RANGE) {
      SLG_REQUIRE(n.n_ranges >= 1, node_name(i) + ": a range node needs at least one range");
      if (n.n_ranges > SLG_MAX_AGG_RANGES)
        throw SlgError(SLG_ERR_UNSUPPORTED, node_name(i) + ": more than SLG_MAX_AGG_RANGES ranges");
      for (uint32_t r = 0; r < n.n_ranges; r++)
        SLG_REQUIRE(!std::isnan(n.from[r]) && !std::isnan(n.to[r]), node_name(i) + ": range bound is NaN");
    }
  }
  for (uint32_t i = 0; i < aggs->n_nodes; i++) {  // (an invalid spec is reported before an unsupported one)
    const slg_agg_node &n = aggs->nodes[i];
    if (n.kind != SLG_AGG_DATE_HISTOGRAM) continue;
    if (!within_two53(n.date_offset))
      throw SlgError(SLG_ERR_UNSUPPORTED, node_name(i) + ": offset beyond +-2^53 ms (CPU path)");
    if (n.has_missing && std::fabs(n.missing) > (double)kTwo53)
      throw SlgError(SLG_ERR_UNSUPPORTED, node_name(i) + ": missing beyond +-2^53 ms (CPU path)");
    if (n.has_hard_bounds && !(within_two53(n.date_hard_min) && within_two53(n.date_hard_max)))
      throw SlgError(SLG_ERR_UNSUPPORTED, node_name(i) + ": hard bound beyond +-2^53 ms (CPU path)");
  }
}

namespace {
// The tables of a checked spec against an index state: the device descriptors, the layout and the cell counts.
// A root's table has root_rows parent rows (1 for an aggregation spec; a composite's children are planned as roots
// under its `size` rows), the count table starts at cell count0 (the composite's own count row lies in front of its
// children's), and cells_before cells of the query are taken already (they count towards SLG_MAX_AGG_CELLS).
struct PlannedTables {
  std::vector<slg::AggNodeDev> nodes;
  std::vector<slg::ColumnDev> cols;
  std::vector<const uint32_t *> rank_cols;
  std::vector<slg_agg_layout> layout;
  uint64_t count_cells = 0, stats_cells = 0, value_cells = 0, card_words = 0, fine_words = 0;
  uint32_t n_value = 0, n_pct = 0, n_walk1 = 0;
};
void plan_tables(const IndexState &S, const slg_agg_spec &aggs, const uint64_t root_rows, const uint64_t count0,
                 const uint64_t cells_before, PlannedTables &P) {
  const size_t n_segs = S.segs.size();
  const uint32_t nn = aggs.n_nodes;
  std::vector<slg::AggNodeDev> &nodes = P.nodes;
  std::vector<slg::ColumnDev> &cols = P.cols;
  std::vector<const uint32_t *> &rank_cols = P.rank_cols;
  std::vector<slg_agg_layout> &layout = P.layout;
  nodes.assign(nn, slg::AggNodeDev{});
  cols.assign((size_t)nn * std::max<size_t>(n_segs, 1), slg::ColumnDev{nullptr, nullptr});
  const std::vector<slgplan::FscoreFieldView> fields = fscore_field_views(S);
  layout.assign(nn, slg_agg_layout{});
  rank_cols.assign((size_t)nn * std::max<size_t>(n_segs, 1), nullptr);
  uint64_t count_cells = count0, stats_cells = 0, value_cells = 0, card_words = 0, fine_words = 0, fine_total = 0;
  uint32_t n_value = 0, n_pct = 0, n_walk1 = 0;
  for (uint32_t i = 0; i < nn; i++) {
    const slg_agg_node &n = aggs.nodes[i];
    // (a filter node has no column: its field is not read — no_field passes the checks below — and its rows of
    // `cols` stay null)
    static const slgplan::FscoreFieldView no_field;
    const bool has_col = n.kind != SLG_AGG_FILTER;
    const slgplan::FscoreFieldView &fd =
        has_col ? slgplan::agg_field(fields, n.field, node_name(i) + ": ", "") : no_field;
    SLG_REQUIRE((n.kind == SLG_AGG_TERMS || (n.kind == SLG_AGG_CARDINALITY && fd.keyword)) == fd.keyword,
                node_name(i) + ": field " + std::to_string(n.field) +
                    (fd.keyword ? " is a keyword field (terms and cardinality only)"
                                : " is a numeric field (not for terms)"));
    if (has_col)
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
    } else if (n.kind == SLG_AGG_FILTER) {
      SLG_REQUIRE((size_t)n.filter < S.filters.size() && S.filter_usable((size_t)n.filter),
                  node_name(i) + ": unknown filter id " + std::to_string(n.filter));
      d.filter = (uint32_t)n.filter;
    } else if (n.kind == SLG_AGG_DATE_HISTOGRAM) {
      d.unit = n.calendar_unit;
      d.step = n.calendar_unit == SLG_DATE_FIXED ? n.date_step : 1;
      d.date_offset = n.date_offset;
      d.has_hard = n.has_hard_bounds ? 1u : 0u;
      d.date_hard_min = n.date_hard_min;
      d.date_hard_max = n.date_hard_max;
      // every collectable value within +-2^53: `as i64` and val - offset are then exact (agg_check_spec saw the
      // offset, `missing` and the hard bounds; an _i64 column that held 2^53 + 1 recorded it as 2^53)
      if (fd.any_value && (fd.i64_rounded || std::fabs(fd.vmin) > (double)kTwo53 || std::fabs(fd.vmax) > (double)kTwo53))
        throw SlgError(SLG_ERR_UNSUPPORTED, node_name(i) + ": agg field " + std::to_string(n.field) +
                                                " holds a value beyond +-2^53 (CPU path)");
      // the dense id range, as the histogram's: date_bucket_id is monotone in the value, and so is `as i64`
      bool any = fd.any_value;
      long long lo = any ? (long long)fd.vmin : 0, hi = any ? (long long)fd.vmax : 0;
      if (n.has_missing) {
        const long long m = (long long)n.missing;
        lo = any ? std::min(lo, m) : m;
        hi = any ? std::max(hi, m) : m;
        any = true;
      }
      if (any && n.has_hard_bounds) {
        lo = std::max(lo, (long long)n.date_hard_min);
        hi = std::min(hi, (long long)n.date_hard_max);
        any = lo <= hi;
      }
      if (any) {
        if (n.calendar_unit != SLG_DATE_FIXED &&
            (lo - n.date_offset < slg::kDateMinMs || hi - n.date_offset > slg::kDateMaxMs))
          throw SlgError(SLG_ERR_UNSUPPORTED, node_name(i) + ": a calendar instant outside 0001-01-01 .. 9999-12-31 "
                                                             "(CPU path)");
        const long long klo = slg::date_bucket_id(d.unit, d.step, d.date_offset, lo);
        const long long khi = slg::date_bucket_id(d.unit, d.step, d.date_offset, hi);
        if (khi - klo + 1 > (long long)SLG_MAX_AGG_CELLS)
          throw SlgError(SLG_ERR_UNSUPPORTED, node_name(i) + ": more than SLG_MAX_AGG_CELLS date_histogram buckets");
        first_id = klo;
        rows = (uint64_t)(khi - klo + 1);
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
    const uint64_t parent_rows = n.parent < 0 ? root_rows : layout[n.parent].rows;
    if (is_value(n.kind)) {
      n_value++;
      d.n_ranges = n.n_ranges;
      std::copy_n(n.from, SLG_MAX_AGG_RANGES, d.from);
      d.shift_from = slg::kAggNoRank;
      const AggFieldData &F = *S.agg_fields.at(n.field);
      uint64_t R = fd.n_ords;
      if (fd.keyword) {  // (cardinality) the ordinals are the ranks
        if (n.has_missing) SLG_REQUIRE(n.missing_ord <= fd.n_ords, node_name(i) + ": missing_ord > n_ords");
        d.miss_rank = n.missing_ord;
        d.n_ranks = fd.n_ords + ((n.has_missing && n.missing_ord == fd.n_ords) ? 1u : 0u);
        for (size_t s = 0; s < n_segs; s++) rank_cols[(size_t)i * n_segs + s] = cols[(size_t)i * n_segs + s].ords();
      } else if (n.kind != SLG_AGG_PERCENTILE_RANKS) {
        if (n.has_missing) SLG_REQUIRE(std::isfinite(n.missing), node_name(i) + ": missing is not finite");
        SLG_REQUIRE(F.dict != nullptr, node_name(i) + ": agg field " + std::to_string(n.field) +
                                           " has no value ranks (slg_index_rank_agg_field)");
        for (size_t s = 0; s < n_segs; s++) {
          SLG_REQUIRE(s < F.ranks.size() && F.ranks[s], node_name(i) + ": agg field " + std::to_string(n.field) +
                                                            " has no value ranks for segment " + std::to_string(s));
          rank_cols[(size_t)i * n_segs + s] = F.ranks[s]->as<const uint32_t>();
        }
        R = F.dict->keys.size();
        d.n_ranks = (uint32_t)R;
        d.dict = F.dict->vals.as<const double>();
        if (n.has_missing) {
          const uint64_t key = f64_key(n.missing);
          const size_t lb = std::lower_bound(F.dict->keys.begin(), F.dict->keys.end(), key) - F.dict->keys.begin();
          d.miss_rank = (uint32_t)lb;
          if (lb == R || F.dict->keys[lb] != key) {  // not a value of the column: one more rank
            d.n_ranks = (uint32_t)R + 1u;
            // cardinality: beyond R; percentiles: a virtual rank at the lower bound, the ranks from there shift
            if (n.kind == SLG_AGG_CARDINALITY) d.miss_rank = (uint32_t)R;
            else d.shift_from = (uint32_t)lb;
          }
        }
      }
      d.n_ranks = std::max(d.n_ranks, 1u);
      if (n.kind == SLG_AGG_CARDINALITY) {
        n_walk1++;
        d.wpr = (d.n_ranks + 31u) / 32u;
        d.bm_off = (uint32_t)card_words;
        card_words += parent_rows * d.wpr;
      } else if (n.kind == SLG_AGG_PERCENTILE_RANKS) {
        n_walk1++;
        rows = 1u + n.n_ranges;
      } else {
        n_pct++;
        rows = 1u + 2u * n.n_ranges;
        const uint32_t lg = ceil_log2(d.n_ranks);
        d.shift = lg > slg::kAggCoarseBits ? lg - slg::kAggCoarseBits : 0u;
        if (d.shift) {  // the fine tables: in the LDS the coarse bins leave behind, or in the scratch slice
          const uint64_t words = (uint64_t)std::min(32u, 2u * n.n_ranges) << d.shift;
          fine_total += words;
          d.fine_lds = words * 4 <= slg::kAggPctLdsBytes ? 1u : 0u;
          if (!d.fine_lds) {
            d.fine_off = (uint32_t)fine_words;  // (behind the bitmaps when those are global too: see below)
            fine_words += words;
          }
        }
      }
      if (card_words + fine_total > SLG_MAX_AGG_SCRATCH_WORDS)
        throw SlgError(SLG_ERR_UNSUPPORTED, "more than SLG_MAX_AGG_SCRATCH_WORDS words of value scratch per query (at " +
                                                node_name(i) + ")");
    }
    uint64_t &cells = is_value(n.kind) ? value_cells : n.kind == SLG_AGG_STATS ? stats_cells : count_cells;
    if (rows > SLG_MAX_AGG_CELLS || parent_rows * rows > SLG_MAX_AGG_CELLS ||
        cells_before + count_cells + stats_cells + value_cells + parent_rows * rows > SLG_MAX_AGG_CELLS)
      throw SlgError(SLG_ERR_UNSUPPORTED, "more than SLG_MAX_AGG_CELLS aggregation cells per query (at " + node_name(i) + ")");
    d.rows = (uint32_t)rows;
    d.first_id = first_id;
    d.off = (uint32_t)cells;
    slg_agg_layout &lay = layout[i];
    lay.parent_rows = (uint32_t)parent_rows;
    lay.rows = (uint32_t)rows;
    lay.first_id = first_id;
    lay.is_stats = is_value(n.kind) ? 2u : n.kind == SLG_AGG_STATS ? 1u : 0u;
    lay.offset = cells;
    cells += parent_rows * rows;
  }
  P.count_cells = count_cells;
  P.stats_cells = stats_cells;
  P.value_cells = value_cells;
  P.card_words = card_words;
  P.fine_words = fine_words;
  P.n_value = n_value;
  P.n_pct = n_pct;
  P.n_walk1 = n_walk1;
}
}  // namespace

// The spec against the batch's index state: fields, the tables' layout, the device descriptors and tables
void slghost::agg_attach(slg_batch *b, const slg_agg_spec &aggs) {
  slg_index *ix = b->idx;
  PlannedTables P;
  plan_tables(*b->snap, aggs, 1, 0, 0, P);
  std::vector<slg::AggNodeDev> &nodes = P.nodes;
  const std::vector<slg::ColumnDev> &cols = P.cols;
  const std::vector<const uint32_t *> &rank_cols = P.rank_cols;
  const uint32_t nn = aggs.n_nodes;
  const uint64_t count_cells = P.count_cells, stats_cells = P.stats_cells, value_cells = P.value_cells,
                 card_words = P.card_words, fine_words = P.fine_words;
  const uint32_t n_value = P.n_value, n_pct = P.n_pct, n_walk1 = P.n_walk1;
  b->agg_layout = P.layout;
  b->aggs = true;
  b->agg_spec = aggs;
  b->agg_count_cells = (uint32_t)count_cells;
  b->agg_stats_cells = (uint32_t)stats_cells;
  b->agg_lds = 4 * count_cells + sizeof(slg::AggStatDev) * stats_cells <= slg::kAggLdsBytes;
  // the value nodes' homes (slg_aggs.hpp): value cells and bitmaps in LDS beside the percentiles region, or global
  b->agg_value_nodes = n_value;
  b->agg_value_cells = (uint32_t)value_cells;
  b->agg_card_words = (uint32_t)card_words;
  b->agg_walk1 = n_walk1 > 0;
  b->agg_ext = false;  // the instantiations with the date_histogram and filter paths
  for (uint32_t i = 0; i < nn; i++)
    b->agg_ext = b->agg_ext || aggs.nodes[i].kind == SLG_AGG_DATE_HISTOGRAM || aggs.nodes[i].kind == SLG_AGG_FILTER;
  b->agg_pct_lds = n_pct ? slg::kAggPctLdsBytes : 0u;
  b->agg_x_lds = 8 * value_cells + 4 * card_words + b->agg_pct_lds <= slg::kAggLdsBytes;
  if (!b->agg_x_lds)
    for (slg::AggNodeDev &d : nodes)
      if (d.kind == SLG_AGG_PERCENTILES && d.shift && !d.fine_lds) d.fine_off += (uint32_t)card_words;
  b->agg_scratch_words = (uint32_t)((b->agg_x_lds ? 0u : card_words) + fine_words);
  upload_image(b->d_agg_desc, &ix->pool, {image_part(nodes), image_part(cols), image_part(rank_cols)});
  const size_t nq = std::max<uint32_t>(b->nq, 1);
  if (n_value) {
    b->d_agg_values.alloc_pooled(&ix->pool, nq * std::max<size_t>(value_cells, 1) * 8);
    b->d_agg_scratch.alloc_pooled(&ix->pool, nq * std::max<size_t>(b->agg_scratch_words, 1) * 4);
  }
  b->d_agg_counts.alloc_pooled(&ix->pool, nq * std::max<size_t>(count_cells, 1) * 4);
  b->d_agg_stats.alloc_pooled(&ix->pool, nq * std::max<size_t>(stats_cells, 1) * sizeof(slg::AggStatDev));
}

CompositeChildTables slghost::agg_plan_children(const IndexState &S, const slg_composite_spec &spec,
                                                const uint64_t cells_before) {
  slg_agg_spec roots{};
  roots.n_nodes = spec.n_children;
  for (uint32_t i = 0; i < spec.n_children; i++) {
    roots.nodes[i] = spec.children[i];
    roots.nodes[i].parent = -1;
  }
  PlannedTables P;
  plan_tables(S, roots, spec.size, spec.size, cells_before, P);
  CompositeChildTables out;
  const ImagePart np = image_part(P.nodes), cp = image_part(P.cols);
  out.nodes.assign(static_cast<const unsigned char *>(np.p), static_cast<const unsigned char *>(np.p) + np.bytes);
  out.cols.assign(static_cast<const unsigned char *>(cp.p), static_cast<const unsigned char *>(cp.p) + cp.bytes);
  out.layout = P.layout;
  out.count_cells = P.count_cells;
  out.stats_cells = P.stats_cells;
  for (uint32_t i = 0; i < spec.n_children; i++)
    out.ext = out.ext || roots.nodes[i].kind == SLG_AGG_DATE_HISTOGRAM || roots.nodes[i].kind == SLG_AGG_FILTER;
  return out;
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
  if (b->agg_value_nodes == p.n_nodes && !p.out_matched) {
    // (nothing but value nodes, and nobody to count for)
  } else if (b->agg_lds) {
    const size_t lds = (size_t)p.stats_cells * sizeof(slg::AggStatDev) + (size_t)p.count_cells * 4;
    launch_kernel_lds(b->agg_ext ? slg::agg_kernel<true, true> : slg::agg_kernel<true, false>, p, dim3(b->nq),
                      slg::kAggThreads, lds, st);
  } else {
    SLG_HIP(hipMemsetAsync(b->d_agg_counts.p, 0, (size_t)b->nq * std::max<size_t>(p.count_cells, 1) * 4, st));
    SLG_HIP(hipMemsetAsync(b->d_agg_stats.p, 0,
                           (size_t)b->nq * std::max<size_t>(p.stats_cells, 1) * sizeof(slg::AggStatDev), st));
    launch_kernel_lds(b->agg_ext ? slg::agg_kernel<false, true> : slg::agg_kernel<false, false>, p, dim3(b->nq),
                      slg::kAggThreads, 0, st);
  }
  if (b->agg_value_nodes == 0) return;
  slg::AggValueParams v{};
  fill_candidates(v, b);
  v.nodes = p.nodes;
  v.cols = p.cols;
  v.rank_cols = reinterpret_cast<const uint32_t *const *>(p.cols + (size_t)p.n_nodes * std::max<size_t>(v.n_segs, 1));
  v.n_nodes = p.n_nodes;
  v.nq = b->nq;
  v.value_cells = b->agg_value_cells;
  v.card_words = b->agg_card_words;
  v.pct_words = b->agg_pct_lds / 4;
  v.scratch_words = b->agg_scratch_words;
  v.walk1 = b->agg_walk1 ? 1u : 0u;
  v.values = b->d_agg_values.as<unsigned long long>();
  v.scratch = b->d_agg_scratch.as<uint32_t>();
  if (v.scratch_words) SLG_HIP(hipMemsetAsync(v.scratch, 0, (size_t)b->nq * v.scratch_words * 4, st));
  if (b->agg_x_lds) {
    const size_t lds = (size_t)b->agg_pct_lds + 8 * (size_t)v.value_cells + 4 * (size_t)v.card_words;
    launch_kernel_lds(b->agg_ext ? slg::agg_values_kernel<true, true> : slg::agg_values_kernel<true, false>, v,
                      dim3(b->nq), slg::kAggThreads, lds, st);
  } else {
    SLG_HIP(hipMemsetAsync(v.values, 0, (size_t)b->nq * std::max<size_t>(v.value_cells, 1) * 8, st));
    launch_kernel_lds(b->agg_ext ? slg::agg_values_kernel<false, true> : slg::agg_values_kernel<false, false>, v,
                      dim3(b->nq), slg::kAggThreads, b->agg_pct_lds, st);
  }
}

extern "C" {

int slg_batch_agg_layout(const slg_batch *b, slg_agg_layout *out) {
  return guarded([&] {
    SLG_REQUIRE(b != nullptr, "batch is NULL");
    SLG_REQUIRE(b->aggs || b->composite || b->term_buckets, "not an aggregation batch (slg_batch_prepare_aggs)");
    if (!b->aggs) return;  // (a composite or term bucket batch without an aggregation spec: no node)
    SLG_REQUIRE(out != nullptr, "out is NULL");
    std::copy(b->agg_layout.begin(), b->agg_layout.end(), out);
  });
}

int slg_batch_fetch_agg_values(slg_batch *b, uint64_t *values) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->aggs, "not an aggregation batch (slg_batch_prepare_aggs)");
    SLG_REQUIRE(b->launched, "the batch has not run");
    const size_t nv = (size_t)b->nq * b->agg_value_cells;
    SLG_REQUIRE(nv == 0 || values != nullptr, "values is NULL");
    if (nv == 0) return;
    DeviceGuard g(b->idx->device);
    const hipStream_t st = locked_stream(b);
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "value cells are 8 bytes");
    SLG_HIP(hipMemcpyAsync(values, b->d_agg_values.p, nv * 8, hipMemcpyDeviceToHost, st));
    SLG_HIP(wait_stream(st));
  });
}

int slg_batch_fetch_aggs(slg_batch *b, uint64_t *counts, slg_agg_stats *stats) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->aggs || b->composite || b->term_buckets, "not an aggregation batch (slg_batch_prepare_aggs)");
    SLG_REQUIRE(b->launched, "the batch has not run");
    // a composite batch: the composite's cells lie behind the spec's in every query's row (tables of their own on
    // the device: agg_kernel's tables keep their stride)
    const size_t ac = agg_spec_cells(b).count, as = agg_spec_cells(b).stats;
    // (a term bucket batch: the same with the children's tables of its nodes; never both kinds in one batch)
    const size_t cc = b->composite ? b->cp_count_cells : b->term_buckets ? b->tb_count_cells : 0u;
    const size_t cs = b->composite ? b->cp_stats_cells : b->term_buckets ? b->tb_stats_cells : 0u;
    const DevBuf &d_cc = b->term_buckets ? b->d_tb_counts : b->d_cp_counts;
    const DevBuf &d_cs = b->term_buckets ? b->d_tb_stats : b->d_cp_stats;
    const size_t nq = b->nq;
    SLG_REQUIRE(nq * (ac + cc) == 0 || counts != nullptr, "counts is NULL");
    SLG_REQUIRE(nq * (as + cs) == 0 || stats != nullptr, "stats is NULL");
    DeviceGuard g(b->idx->device);
    const hipStream_t st = locked_stream(b);
    std::vector<uint32_t> hc(nq * ac), hcc(nq * cc);
    std::vector<slg::AggStatDev> hs(nq * as), hcs(nq * cs);
    if (!hc.empty()) SLG_HIP(hipMemcpyAsync(hc.data(), b->d_agg_counts.p, hc.size() * 4, hipMemcpyDeviceToHost, st));
    if (!hs.empty())
      SLG_HIP(hipMemcpyAsync(hs.data(), b->d_agg_stats.p, hs.size() * sizeof(slg::AggStatDev), hipMemcpyDeviceToHost, st));
    if (!hcc.empty()) SLG_HIP(hipMemcpyAsync(hcc.data(), d_cc.p, hcc.size() * 4, hipMemcpyDeviceToHost, st));
    if (!hcs.empty())
      SLG_HIP(hipMemcpyAsync(hcs.data(), d_cs.p, hcs.size() * sizeof(slg::AggStatDev), hipMemcpyDeviceToHost, st));
    SLG_HIP(wait_stream(st));
    auto value = [](unsigned long long key) {  // the inverse of agg_f64_key
      const unsigned long long bits = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
      double x;
      std::memcpy(&x, &bits, 8);
      return x;
    };
    auto stat = [&](const slg::AggStatDev &h, slg_agg_stats &o) {
      o = slg_agg_stats{0, 0.0, 0.0, 0.0};  // StatsState::default
      if (h.count == 0) return;
      o.count = h.count;
      o.min = value(~h.min_key);
      o.max = value(h.max_key);
      o.sum = h.sum;
    };
    for (size_t q = 0; q < nq; q++) {
      for (size_t i = 0; i < ac; i++) counts[q * (ac + cc) + i] = hc[q * ac + i];
      for (size_t i = 0; i < cc; i++) counts[q * (ac + cc) + ac + i] = hcc[q * cc + i];
      for (size_t i = 0; i < as; i++) stat(hs[q * as + i], stats[q * (as + cs) + i]);
      for (size_t i = 0; i < cs; i++) stat(hcs[q * cs + i], stats[q * (as + cs) + as + i]);
    }
  });
}

}  // extern "C"
