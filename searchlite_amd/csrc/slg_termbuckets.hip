// slg_termbuckets.hip — significant_terms / rare_terms batches (slg_batch_prepare_term_buckets): the checks of a spec,
// the nodes against the batch's index state (keyword columns, background filters, ranks), the background tables
// (bg_count_kernel, at prepare), the children's tables (planned by slg_aggs.hip as the roots of `size` parent rows),
// the launches of term_bucket_count_kernel, term_bucket_select_kernel and term_bucket_collect_kernel behind
// agg_kernel, and slg_batch_term_buckets_layout / _fetch_term_buckets.
// (The spec checks live in this .hip unit, as composite's do: the host sanitizer harness does not reach them.)
#include "slg_host.hpp"

#include <map>

#include "slg_termbuckets.hpp"

using namespace slghost;

static_assert(slg::kTbMaxNodes == SLG_MAX_TERM_BUCKET_NODES && slg::kTbMaxSize == SLG_MAX_TERM_BUCKET_SIZE &&
                  slg::kTbMaxSize <= slg::kCpMaxSize,
              "the kernel's limits and the ABI's");
static_assert(slg::kTbSignificant == SLG_TERMS_SIGNIFICANT && slg::kTbRare == SLG_TERMS_RARE, "node kinds");
static_assert(sizeof(slg::TermBucketNodeDev) % 8 == 0 && sizeof(slg::AggNodeDev) % 8 == 0, "records of whole words");

namespace {
std::string tb_name(uint32_t i) { return "term bucket node " + std::to_string(i); }
bool is_value_kind(int32_t kind) {
  return kind == SLG_AGG_CARDINALITY || kind == SLG_AGG_PERCENTILES || kind == SLG_AGG_PERCENTILE_RANKS;
}
// d_tb_out: u64 doc_counts, bg_counts, score_bits [nq * rows], node_dc, node_bg [nq * n]; then u32 ords [nq * rows],
// n_buckets [nq * n], the error word
struct OutBlock {
  size_t nq, rows, n;
  OutBlock(const slg_batch *b)
      : nq(std::max<uint32_t>(b->nq, 1)), rows(b->tb_layout.rows), n(b->tb_spec.n_nodes) {}
  size_t u64s() const { return 3 * nq * rows + 2 * nq * n; }
  size_t words() const { return 2 * u64s() + nq * rows + nq * n + 1; }
};
// the children of one node as a composite's: agg_plan_children plans them under `size` parent rows
slg_composite_spec children_as_composite(const slg_term_bucket_node &n) {
  slg_composite_spec cs{};
  cs.size = n.size;
  cs.n_children = n.n_children;
  for (uint32_t c = 0; c < n.n_children; c++) cs.children[c] = n.children[c];
  return cs;
}
}  // namespace

void slghost::term_buckets_check_spec(const slg_term_bucket_spec *spec) {
  SLG_REQUIRE(spec != nullptr, "term bucket spec is NULL");
  SLG_REQUIRE(spec->n_nodes >= 1, "a term bucket spec needs at least one node");
  const uint32_t nn = std::min<uint32_t>(spec->n_nodes, SLG_MAX_TERM_BUCKET_NODES);
  std::string unsupported;
  for (uint32_t i = 0; i < nn; i++) {
    const slg_term_bucket_node &n = spec->nodes[i];
    SLG_REQUIRE(n.kind == SLG_TERMS_SIGNIFICANT || n.kind == SLG_TERMS_RARE, tb_name(i) + ": unknown kind");
    SLG_REQUIRE(n.background_filter >= -1, tb_name(i) + ": background_filter < -1");
    SLG_REQUIRE(n.kind == SLG_TERMS_SIGNIFICANT || n.background_filter == -1,
                tb_name(i) + ": a rare_terms node has no background_filter");
    // the children as slg_batch_prepare_aggs would see them as roots (an invalid child is reported before anything
    // unsupported)
    const uint32_t nc = std::min<uint32_t>(n.n_children, SLG_MAX_AGGS);
    if (nc) {
      slg_agg_spec roots{};
      roots.n_nodes = nc;
      for (uint32_t c = 0; c < nc; c++) {
        roots.nodes[c] = n.children[c];
        roots.nodes[c].parent = -1;
      }
      try {
        agg_check_spec(&roots);
      } catch (const SlgError &e) {
        const std::string msg = tb_name(i) + " child: " + e.what();
        if (e.code != SLG_ERR_UNSUPPORTED) throw SlgError(e.code, msg);
        if (unsupported.empty()) unsupported = msg;
      }
    }
  }
  if (spec->n_nodes > SLG_MAX_TERM_BUCKET_NODES)
    throw SlgError(SLG_ERR_UNSUPPORTED, "more than SLG_MAX_TERM_BUCKET_NODES term bucket nodes");
  for (uint32_t i = 0; i < nn; i++) {
    const slg_term_bucket_node &n = spec->nodes[i];
    if (n.size == 0)
      throw SlgError(SLG_ERR_UNSUPPORTED, tb_name(i) + ": size is 0 (all buckets: CPU path)");
    if (n.size > SLG_MAX_TERM_BUCKET_SIZE)
      throw SlgError(SLG_ERR_UNSUPPORTED, tb_name(i) + ": size > SLG_MAX_TERM_BUCKET_SIZE");
    if (n.n_children > SLG_MAX_AGGS)
      throw SlgError(SLG_ERR_UNSUPPORTED, tb_name(i) + ": more than SLG_MAX_AGGS children");
  }
  if (!unsupported.empty()) throw SlgError(SLG_ERR_UNSUPPORTED, unsupported);
  for (uint32_t i = 0; i < nn; i++)
    for (uint32_t c = 0; c < spec->nodes[i].n_children; c++)
      if (is_value_kind(spec->nodes[i].children[c].kind))
        throw SlgError(SLG_ERR_UNSUPPORTED, tb_name(i) + " child " + std::to_string(c) +
                                                ": cardinality, percentiles and percentile_ranks are not built under a "
                                                "term bucket node (CPU path)");
}

void slghost::term_buckets_attach(slg_batch *b, const slg_term_bucket_spec &spec) {
  const IndexState &S = *b->snap;
  slg_index *ix = b->idx;
  const size_t n_segs = S.segs.size();
  const uint32_t nn = spec.n_nodes;
  const std::vector<slgplan::FscoreFieldView> fields = fscore_field_views(S);
  std::vector<const slgplan::FscoreFieldView *> fds(nn, nullptr);
  std::vector<slg::ColumnDev> cols((size_t)nn * std::max<size_t>(n_segs, 1), slg::ColumnDev{nullptr, nullptr});
  std::vector<uint32_t> ranks;  // per ranked node: ord_rank, then its inverse
  std::vector<size_t> rank_at(nn, ~(size_t)0);
  for (uint32_t i = 0; i < nn; i++) {  // what is invalid, for every node, before what is unsupported
    const slg_term_bucket_node &n = spec.nodes[i];
    const slgplan::FscoreFieldView &fd = slgplan::agg_field(fields, n.field, tb_name(i) + ": ", "");
    fds[i] = &fd;
    std::copy_n(slgplan::agg_field_rows(fd, (uint32_t)n_segs, tb_name(i) + ": ", ""), n_segs,
                cols.begin() + (size_t)i * n_segs);
    SLG_REQUIRE(fd.keyword, tb_name(i) + ": field " + std::to_string(n.field) + " is a numeric field (a keyword column only)");
    if (n.background_filter >= 0)
      SLG_REQUIRE(S.filter_usable((size_t)n.background_filter),
                  tb_name(i) + ": unknown filter id " + std::to_string(n.background_filter));
    if (n.ord_rank) {
      std::vector<uint32_t> inv(fd.n_ords, 0u);
      std::vector<char> seen(fd.n_ords, 0);
      for (uint32_t o = 0; o < fd.n_ords; o++) {
        const uint32_t r = n.ord_rank[o];
        SLG_REQUIRE(r < fd.n_ords && !seen[r], tb_name(i) + ": ord_rank is not a permutation of [0, n_ords)");
        seen[r] = 1;
        inv[r] = o;
      }
      rank_at[i] = ranks.size();
      ranks.insert(ranks.end(), n.ord_rank, n.ord_rank + fd.n_ords);
      ranks.insert(ranks.end(), inv.begin(), inv.end());
    }
  }
  // the tables: per node n_ords foreground and n_ords background-sum cells, the presence words of a significant
  // node, `size` output rows; with children `size` count cells and the children's tables, behind the cells of the
  // aggregation spec in a query's rows
  const AggSpecCells spec_cells = agg_spec_cells(b);
  const uint64_t agg_cells = spec_cells.all();
  slg_term_bucket_layout lay{};
  lay.n_nodes = nn;
  std::vector<slg::TermBucketNodeDev> nodes(nn);
  uint64_t fg_cells = 0, bits_words = 0, rows = 0;
  for (uint32_t i = 0; i < nn; i++) {
    const slg_term_bucket_node &n = spec.nodes[i];
    slg::TermBucketNodeDev &d = nodes[i];
    d = slg::TermBucketNodeDev{};
    d.kind = n.kind;
    d.size = n.size;
    d.n_ords = fds[i]->n_ords;
    d.cap = slg::cp_cap(n.size);
    d.bound = n.doc_count_bound;
    d.fg_off = (uint32_t)fg_cells;
    d.row_off = (uint32_t)rows;
    d.n_children = n.n_children;
    fg_cells += d.n_ords;
    rows += n.size;
    if (n.kind == SLG_TERMS_SIGNIFICANT) {
      d.wpr = (d.n_ords + 31u) / 32u;
      d.bits_off = (uint32_t)bits_words;
      bits_words += (uint64_t)n_segs * d.wpr;
    }
    if (agg_cells + 2 * fg_cells > SLG_MAX_AGG_CELLS)
      throw SlgError(SLG_ERR_UNSUPPORTED, "more than SLG_MAX_AGG_CELLS aggregation cells per query (at " + tb_name(i) + ")");
    if (bits_words > SLG_MAX_AGG_SCRATCH_WORDS)
      throw SlgError(SLG_ERR_UNSUPPORTED,
                     "more than SLG_MAX_AGG_SCRATCH_WORDS words of presence bits per query (at " + tb_name(i) + ")");
    lay.nodes[i].size = n.size;
    lay.nodes[i].n_children = n.n_children;
    lay.nodes[i].row_offset = d.row_off;
  }
  lay.rows = (uint32_t)rows;
  const uint32_t ac = spec_cells.count, as = spec_cells.stats;
  std::vector<CompositeChildTables> ch(nn);
  uint64_t count_cells = 0, stats_cells = 0;
  for (uint32_t i = 0; i < nn; i++) {
    slg_batch::TbNodeTables &T = b->tb_tables[i];
    T = slg_batch::TbNodeTables{};
    if (spec.nodes[i].n_children == 0) continue;
    try {
      ch[i] = agg_plan_children(S, children_as_composite(spec.nodes[i]),
                                agg_cells + 2 * fg_cells + count_cells + stats_cells);
    } catch (const SlgError &e) {
      throw SlgError(e.code, tb_name(i) + " child: " + e.what());
    }
    T.cnt_off = (uint32_t)count_cells;
    T.st_off = (uint32_t)stats_cells;
    T.count_cells = (uint32_t)ch[i].count_cells;
    T.stats_cells = (uint32_t)ch[i].stats_cells;
    T.lds = 4 * ch[i].count_cells + sizeof(slg::AggStatDev) * ch[i].stats_cells + 8ull * spec.nodes[i].size <=
            slg::kAggLdsBytes;
    T.ext = ch[i].ext;
    lay.nodes[i].count_offset = ac + count_cells;
    for (uint32_t c = 0; c < spec.nodes[i].n_children; c++) {
      lay.nodes[i].children[c] = ch[i].layout[c];
      lay.nodes[i].children[c].offset += lay.nodes[i].children[c].is_stats ? as + stats_cells : ac + count_cells;
    }
    count_cells += ch[i].count_cells;
    stats_cells += ch[i].stats_cells;
  }
  b->term_buckets = true;
  b->tb_spec = spec;
  for (uint32_t i = 0; i < SLG_MAX_TERM_BUCKET_NODES; i++) b->tb_spec.nodes[i].ord_rank = nullptr;
  b->tb_layout = lay;
  b->tb_fg_cells = (uint32_t)fg_cells;
  b->tb_bits_words = (uint32_t)bits_words;
  b->tb_count_cells = (uint32_t)count_cells;
  b->tb_stats_cells = (uint32_t)stats_cells;
  b->tb_lds = 4 * fg_cells <= slg::kAggLdsBytes;

  if (!ranks.empty()) {
    b->d_tb_ranks.alloc_pooled(&ix->pool, ranks.size() * 4);
    SLG_HIP(hipMemcpy(b->d_tb_ranks.p, ranks.data(), ranks.size() * 4, hipMemcpyHostToDevice));
  }
  // the background: one table [n_segs][n_ords + 1] per distinct (field, filter) of the significant nodes
  std::map<std::pair<int32_t, int32_t>, size_t> bg_at;
  size_t bg_words = 0;
  for (uint32_t i = 0; i < nn; i++) {
    if (spec.nodes[i].kind != SLG_TERMS_SIGNIFICANT) continue;
    const auto key = std::make_pair(spec.nodes[i].field, spec.nodes[i].background_filter);
    if (bg_at.emplace(key, bg_words).second) bg_words += n_segs * ((size_t)nodes[i].n_ords + 1);
  }
  if (bg_words) {
    b->d_tb_bg.alloc_pooled(&ix->pool, bg_words * 4);
    SLG_HIP(hipMemset(b->d_tb_bg.p, 0, bg_words * 4));
    std::map<std::pair<int32_t, int32_t>, bool> done;
    for (uint32_t i = 0; i < nn; i++) {
      if (spec.nodes[i].kind != SLG_TERMS_SIGNIFICANT) continue;
      const auto key = std::make_pair(spec.nodes[i].field, spec.nodes[i].background_filter);
      if (done[key]) continue;
      done[key] = true;
      const uint32_t n_ords = nodes[i].n_ords;
      for (size_t s = 0; s < n_segs; s++) {
        slg::BgCountParams p{};
        p.col = cols[(size_t)i * n_segs + s];
        p.deleted = S.segs[s]->d_deleted.as<const uint32_t>();
        p.reject = key.second >= 0 ? S.reject_host[(size_t)key.second * n_segs + s] : nullptr;
        p.n_docs = S.segs[s]->n_docs;
        p.n_ords = n_ords;
        p.bg = b->d_tb_bg.as<uint32_t>() + bg_at[key] + s * ((size_t)n_ords + 1);
        if (p.n_docs == 0) continue;
        const uint32_t blocks =
            std::min<uint32_t>((p.n_docs + slg::kTbThreads - 1) / slg::kTbThreads, slg::kTbBgBlocks);
        // (the null stream, waited for below: the tables are complete before the batch can run on any stream)
        if ((size_t)n_ords * 4 <= slg::kAggLdsBytes)
          launch_kernel_lds(slg::bg_count_kernel<true>, p, dim3(blocks), slg::kTbThreads, (size_t)n_ords * 4, nullptr);
        else
          launch_kernel_lds(slg::bg_count_kernel<false>, p, dim3(blocks), slg::kTbThreads, 0, nullptr);
      }
    }
    SLG_HIP(hipStreamSynchronize(nullptr));
  }
  for (uint32_t i = 0; i < nn; i++) {
    if (rank_at[i] != ~(size_t)0) {
      nodes[i].ord_rank = b->d_tb_ranks.as<const uint32_t>() + rank_at[i];
      nodes[i].rank_ord = nodes[i].ord_rank + nodes[i].n_ords;
    }
    if (spec.nodes[i].kind == SLG_TERMS_SIGNIFICANT)
      nodes[i].bg = b->d_tb_bg.as<const uint32_t>() +
                    bg_at[std::make_pair(spec.nodes[i].field, spec.nodes[i].background_filter)];
  }
  // the image: the nodes, their columns, then every node's children (AggNodeDev[], ColumnDev[])
  std::vector<ImagePart> parts{image_part(nodes), image_part(cols)};
  size_t at = nodes.size() * sizeof(slg::TermBucketNodeDev) + cols.size() * sizeof(slg::ColumnDev);
  b->tb_cols_off = nodes.size() * sizeof(slg::TermBucketNodeDev);
  for (uint32_t i = 0; i < nn; i++) {
    b->tb_tables[i].nodes_off = at;
    b->tb_tables[i].cols_off = at + ch[i].nodes.size();
    at += ch[i].nodes.size() + ch[i].cols.size();
    parts.push_back(ImagePart{ch[i].nodes.data(), ch[i].nodes.size()});
    parts.push_back(ImagePart{ch[i].cols.data(), ch[i].cols.size()});
  }
  {
    std::vector<unsigned char> image;
    for (const ImagePart &pt : parts)
      image.insert(image.end(), static_cast<const unsigned char *>(pt.p), static_cast<const unsigned char *>(pt.p) + pt.bytes);
    b->d_tb_desc.alloc_pooled(&ix->pool, image.size());
    SLG_HIP(hipMemcpy(b->d_tb_desc.p, image.data(), image.size(), hipMemcpyHostToDevice));
  }
  const size_t nq = std::max<uint32_t>(b->nq, 1);
  b->d_tb_fg.alloc_pooled(&ix->pool, nq * std::max<size_t>(fg_cells, 1) * 4);
  b->d_tb_bgsum.alloc_pooled(&ix->pool, nq * std::max<size_t>(fg_cells, 1) * 8);
  b->d_tb_bits.alloc_pooled(&ix->pool, nq * std::max<size_t>(bits_words, 1) * 4);
  b->d_tb_out.alloc_pooled(&ix->pool, OutBlock(b).words() * 4);
  b->d_tb_sorted.alloc_pooled(&ix->pool, 2 * nq * std::max<size_t>(rows, 1) * 4);
  b->d_tb_counts.alloc_pooled(&ix->pool, nq * std::max<size_t>(count_cells, 1) * 4);
  b->d_tb_stats.alloc_pooled(&ix->pool, nq * std::max<size_t>(stats_cells, 1) * sizeof(slg::AggStatDev));
}

void slghost::term_buckets_launch(slg_batch *b, hipStream_t st) {
  if (b->nq == 0) return;
  const size_t nq = b->nq;
  const OutBlock O(b);
  slg::TermBucketParams p{};
  fill_candidates(p.a, b);
  p.a.nq = b->nq;
  unsigned char *const desc = b->d_tb_desc.as<unsigned char>();
  p.tb = reinterpret_cast<const slg::TermBucketNodeDev *>(desc);
  p.tb_cols = reinterpret_cast<const slg::ColumnDev *>(desc + b->tb_cols_off);
  p.n_tb = b->tb_spec.n_nodes;
  p.fg_cells = b->tb_fg_cells;
  p.bits_words = b->tb_bits_words;
  p.rows = b->tb_layout.rows;
  p.cnt_stride = b->tb_count_cells;
  p.st_stride = b->tb_stats_cells;
  p.fg = b->d_tb_fg.as<uint32_t>();
  p.bgsum = b->d_tb_bgsum.as<unsigned long long>();
  p.bits = b->d_tb_bits.as<uint32_t>();
  unsigned long long *const o64 = b->d_tb_out.as<unsigned long long>();
  p.doc_counts = o64;
  p.bg_counts = o64 + O.nq * O.rows;
  p.score_bits = o64 + 2 * O.nq * O.rows;
  p.node_dc = o64 + 3 * O.nq * O.rows;
  p.node_bg = p.node_dc + O.nq * O.n;
  p.ords = reinterpret_cast<uint32_t *>(o64 + O.u64s());
  p.n_buckets = p.ords + O.nq * O.rows;
  p.err = p.n_buckets + O.nq * O.n;
  p.sorted_ords = b->d_tb_sorted.as<uint32_t>();
  p.row_of = p.sorted_ords + O.nq * std::max<size_t>(O.rows, 1);
  p.flag = ResultBlock(b->nq, b->k).flag(b->d_out.as<uint32_t>());
  // a sorted batch's select counted the accepted docs, agg_kernel does in score order; without either the count walk
  p.a.out_matched = post_select_matched(b);
  if (p.bits_words) {  // (a significant node: the presence words and the sums they guard)
    SLG_HIP(hipMemsetAsync(p.bgsum, 0, nq * std::max<size_t>(p.fg_cells, 1) * 8, st));
    SLG_HIP(hipMemsetAsync(p.bits, 0, nq * (size_t)p.bits_words * 4, st));
  }
  if (b->tb_lds) {
    launch_kernel_lds(slg::term_bucket_count_kernel<true>, p, dim3(b->nq), slg::kTbThreads, 4 * (size_t)p.fg_cells, st);
  } else {
    SLG_HIP(hipMemsetAsync(p.fg, 0, nq * std::max<size_t>(p.fg_cells, 1) * 4, st));
    launch_kernel_lds(slg::term_bucket_count_kernel<false>, p, dim3(b->nq), slg::kTbThreads, 0, st);
  }
  uint32_t cap = slg::kCpMinCap;
  for (uint32_t i = 0; i < p.n_tb; i++) cap = std::max(cap, slg::cp_cap(b->tb_spec.nodes[i].size));
  launch_kernel_lds(slg::term_bucket_select_kernel, p, dim3(b->nq, p.n_tb), slg::kTbThreads,
                    (size_t)slg::kCpWaves * cap * 8, st);
  bool any_global = false;  // (one memset of the whole tables for the nodes in the global home)
  for (uint32_t i = 0; i < p.n_tb; i++)
    any_global = any_global || (b->tb_spec.nodes[i].n_children != 0 && !b->tb_tables[i].lds);
  if (any_global) {
    SLG_HIP(hipMemsetAsync(b->d_tb_counts.p, 0, nq * std::max<size_t>(b->tb_count_cells, 1) * 4, st));
    SLG_HIP(hipMemsetAsync(b->d_tb_stats.p, 0, nq * std::max<size_t>(b->tb_stats_cells, 1) * sizeof(slg::AggStatDev), st));
  }
  for (uint32_t i = 0; i < p.n_tb; i++) {
    const slg_batch::TbNodeTables &T = b->tb_tables[i];
    if (b->tb_spec.nodes[i].n_children == 0) continue;
    slg::TermBucketParams c = p;
    c.node = i;
    c.a.nodes = reinterpret_cast<const slg::AggNodeDev *>(desc + T.nodes_off);
    c.a.cols = reinterpret_cast<const slg::ColumnDev *>(desc + T.cols_off);
    c.a.n_nodes = b->tb_spec.nodes[i].n_children;
    c.a.count_cells = T.count_cells;
    c.a.stats_cells = T.stats_cells;
    c.a.counts = b->d_tb_counts.as<uint32_t>() + T.cnt_off;
    c.a.stats = b->d_tb_stats.as<slg::AggStatDev>() + T.st_off;
    const size_t ord_lds = 8 * (size_t)b->tb_spec.nodes[i].size;
    if (T.lds) {
      const size_t lds = ord_lds + (size_t)T.stats_cells * sizeof(slg::AggStatDev) + (size_t)T.count_cells * 4;
      launch_kernel_lds(T.ext ? slg::term_bucket_collect_kernel<true, true> : slg::term_bucket_collect_kernel<true, false>,
                        c, dim3(b->nq), slg::kTbThreads, lds, st);
    } else {
      launch_kernel_lds(T.ext ? slg::term_bucket_collect_kernel<false, true> : slg::term_bucket_collect_kernel<false, false>,
                        c, dim3(b->nq), slg::kTbThreads, ord_lds, st);
    }
  }
}

extern "C" {

int slg_batch_term_buckets_layout(const slg_batch *b, slg_term_bucket_layout *out) {
  return guarded([&] {
    SLG_REQUIRE(b != nullptr, "batch is NULL");
    SLG_REQUIRE(b->term_buckets, "not a term bucket batch (slg_batch_prepare_term_buckets)");
    SLG_REQUIRE(out != nullptr, "out is NULL");
    *out = b->tb_layout;
  });
}

int slg_batch_fetch_term_buckets(slg_batch *b, uint32_t *ords, uint64_t *doc_counts, uint64_t *bg_counts,
                                 uint64_t *score_bits, uint32_t *n_buckets, uint64_t *node_doc_count,
                                 uint64_t *node_bg_count) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->term_buckets, "not a term bucket batch (slg_batch_prepare_term_buckets)");
    SLG_REQUIRE(b->launched, "the batch has not run");
    DeviceGuard g(b->idx->device);
    const hipStream_t st = locked_stream(b);
    if (b->nq == 0) return;
    // the arrays and the error word behind them are one block
    const OutBlock O(b);
    const size_t words = O.words(), nr = O.nq * O.rows, nn = O.nq * O.n;
    const SideBlock host(b, b->d_tb_out, words, st);
    const uint32_t *const blk = host.p;
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "8-byte cells");
    const uint32_t *u64s = blk;
    if (doc_counts) std::memcpy(doc_counts, u64s, nr * 8);
    if (bg_counts) std::memcpy(bg_counts, u64s + 2 * nr, nr * 8);
    if (score_bits) std::memcpy(score_bits, u64s + 4 * nr, nr * 8);
    if (node_doc_count) {
      std::memcpy(node_doc_count, u64s + 6 * nr, nn * 8);
      for (size_t q = 0; q < O.nq; q++)  // (a rare node returns no totals)
        for (size_t i = 0; i < O.n; i++)
          if (b->tb_spec.nodes[i].kind == SLG_TERMS_RARE) node_doc_count[q * O.n + i] = 0;
    }
    if (node_bg_count) std::memcpy(node_bg_count, u64s + 6 * nr + 2 * nn, nn * 8);
    const uint32_t *u32s = blk + 2 * O.u64s();
    if (ords) std::memcpy(ords, u32s, nr * 4);
    if (n_buckets) std::memcpy(n_buckets, u32s + nr, nn * 4);
  });
}

}  // extern "C"
