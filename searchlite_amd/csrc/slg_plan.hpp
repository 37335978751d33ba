// slg_plan.hpp — the host planner of a query batch: a PURE function of the segments' host mirrors,
// the index's tuning and the caller's query arrays -> the descriptor image the kernels consume
// (sub-queries, term references, slices, launch order).  No HIP in here: the translation unit
// builds with g++ and is unit-tested and sanitized on a box without a GPU
// (tests/test_plan.py, tools/sanitize_cpu.sh; tools/plan_digest.cpp beside this file is a stand-alone
// driver that digests everything plan_batch returns over a fixed list of batches: two builds of the
// planner are compared, or one is run under a sanitizer, with it); slg_batch.hip uploads what it returns.
//
// What it mirrors: IndexReader::search_segment's preparation of the scorer call
// (searchlite-core/src/api/reader.rs:2971-3005: ScoredTerm list per segment, terms with empty
// postings dropped wand.rs:441), the score plan's shape (query/planner.rs:113-153), and the
// decisions the reference's cursors take while running (wand.rs:107-153 upper bounds ->
// here: threshold seed and MaxScore classification from the champion table).
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/searchlite_gpu.h"
#include "slg_desc.hpp"

namespace slgplan {

struct SlgError : std::runtime_error {
  int code;
  SlgError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

// host mirror of one staged segment
struct SegView {
  uint32_t n_docs = 0, n_terms = 0;
  const uint64_t *term_offsets = nullptr;  // [n_terms + 1] as given (unpadded)
  const float *champ = nullptr;            // [n_terms * kChampions] or nullptr (champions off)
  bool has_positions = false;              // slg_index_set_positions was called for it (phrase batches)
};

// the caller's arrays (slg_batch_prepare_plans)
struct BatchIn {
  uint32_t nq = 0;
  const uint32_t *q_offsets = nullptr;
  const uint32_t *q_term_ids = nullptr;
  const float *q_weights = nullptr;
  slg_score_plans plans{};            // all-NULL: term i of a query is leaf i, summed
  const int32_t *q_filter = nullptr;
  uint32_t k = 0;
  int strategy = SLG_STRATEGY_WAND;
  const char *filter_live = nullptr;  // [n_filters] 1 = the filter id is registered
  size_t n_filters = 0;
  // field-sorted batch (slg_batch_prepare_sorted) or cursor batch (slg_batch_prepare_after, both orders):
  // every matched doc is a candidate with its exact score, whatever k is — candidates mode, no threshold
  // seed, no MaxScore classification (the seed bounds the k-th score over ALL docs; after a cursor the
  // k-th eligible score is lower, and a seed or a prune would drop docs of the page)
  bool sorted = false;
};

// k the batch is planned (and its scoring kernel launched) with: a sorted batch runs as a large-k batch
// (> 1024: candidates mode and no seed), whatever k it returns
constexpr uint32_t kSortedPlanK = 1025;
inline uint32_t planning_k(const BatchIn &in) { return in.sorted && in.k < kSortedPlanK ? kSortedPlanK : in.k; }

// ---- sort keys of numeric fast fields (slg_index_add_sort_field_*) ----
// query/sort.rs:300-345: the value of a field part is min_by (Asc) / max_by (Desc) of the doc's values under
// partial_cmp(..).unwrap_or(Equal) — min_by keeps the first of "equal" elements, max_by the last — and a doc
// without values is Missing.  Per doc this writes the value's order-preserving u64 under each order (asc:
// ascending i64 / f64 total_cmp order; desc: the complement of the same, so ascending u64 order is the sort
// order in both) and a presence bit (bit d & 31 of word d >> 5; clear = Missing, whose keys are 0).
// offsets == NULL: every doc is Missing.  kind: 1 i64, 2 f64.
void sort_field_keys(int kind, uint32_t n_docs, const uint32_t *offsets, const void *values, uint64_t *asc,
                     uint64_t *desc, uint32_t *present_words);

// ---- cursor keys (slg_batch_prepare_after) ----
// The cursor's key as the words the select kernels compare.  n_parts == 0: score order -> out[0..2] =
// (ordered score, ~segment, ~doc), descending as select_topk_kernel's candidate keys.  Otherwise a field sort
// (kind[p]: 0 `_score`, 1 i64, 2 f64; order[p] SLG_ORDER_*) -> out[0..kCursorWords-1] ascending as
// select_sorted_kernel's keys: per part (missing flag, u64 key high, low) — the column encoding of
// sort_field_keys applied to the cursor's value itself (the reference already picked it: no min_by / max_by),
// complemented for Desc; a `_score` part is (0, 0, ordered score, complemented for Desc) — zero words for
// parts beyond the spec, then segment, doc.  Throws SlgError(SLG_ERR_INVALID) for a Missing bit on a
// `_score` part or beyond the spec, non-zero value_bits beyond the spec, or a `_score` value above 32 bits.
constexpr uint32_t kCursorWords = 3 * SLG_MAX_SORT_PARTS + 2;
void cursor_key(uint32_t n_parts, const int *kind, const int32_t *order, const slg_sort_cursor &c, uint32_t *out);

struct Plan {
  // ---- the descriptor image ----
  std::vector<slg::RoundQuery> sqs;
  std::vector<slg::TermRef> terms;
  std::vector<uint32_t> slice_sq, slice_seg, slice_order;
  std::vector<slg::QueryRef> qrefs;
  std::vector<uint32_t> bnd_coarse;  // sub-query of every 32nd round boundary
  std::vector<slg::PlanNode> nodes;  // canonical node tables of the queries with deep score trees
  std::vector<uint32_t> q_filter;    // [nq] 0 = none, f + 1 (empty when no query is filtered)
  // ---- accounting ----
  std::vector<uint64_t> q_postings;  // per query (stats.postings_advanced)
  uint64_t n_postings = 0, n_postings_essential = 0, n_postings_nonessential = 0;
  uint64_t n_rounds = 0, n_bounds = 0, n_bnd = 0, cand_total = 0;
  uint32_t max_terms = 0;
  // ---- what runs ----
  bool uniform = false;     // every sub-query fits the few-term kernel
  bool multi = false;       // many-term kernel
  bool plan_batch = false;  // some sub-query has a score plan
  bool nested = false;      // some sub-query has a two-level plan (groups of leaves)
  bool deep = false;        // some sub-query has a score tree of more than two levels
  bool pruned = false;      // some sub-query has non-essential lists (MaxScore)
  bool cand_mode = false;   // k > 256 on candidates + select
  // ---- packed image layout (pack()) ----
  size_t o_sq = 0, o_terms = 0, o_slice = 0, o_sseg = 0, o_sord = 0, o_q = 0, o_bc = 0, o_nodes = 0, image_bytes = 0;
  void layout();
  void pack(unsigned char *dst) const;  // dst: image_bytes bytes
};

// ---- query rescore (slg_batch_prepare_rescore) ----
// The checks of a rescore spec that need no index (throws SlgError): NULL spec or arrays, offsets, term
// counts, modes, plans, ties, weights (SLG_ERR_INVALID), windows that, capped at k, exceed the limit
// (SLG_ERR_UNSUPPORTED).
void check_rescore(const slg_rescore_spec *spec, uint32_t nq, uint32_t k);
// The per-(query, segment) term table of a checked spec against the segments (slg::RescoreQuery /
// RescoreTerm: slg_desc.hpp).  Throws SLG_ERR_INVALID for a term id out of range, SLG_ERR_UNSUPPORTED
// for a query whose table exceeds slg::kRescoreMaxTable entries.
struct RescorePlan {
  std::vector<slg::RescoreQuery> queries;  // [nq]
  std::vector<slg::RescoreTerm> terms;     // [total x n_segs]
  uint32_t max_window = 0;                 // the largest min(window, k) of a query with terms
  uint32_t max_table = 0;                  // the most table entries (terms x segments) of a query
};
void plan_rescore(const std::vector<SegView> &segs, uint32_t nq, uint32_t k, const slg_rescore_spec &spec,
                  RescorePlan &out);

// ---- field collapsing (slg_batch_prepare_collapse) ----
// The checks of a collapse spec that need no index (throws SlgError): a NULL spec, group_limit outside 1 .. k,
// an inner sort part with an unknown order or a negative field other than SLG_SORT_SCORE (SLG_ERR_INVALID,
// reported first); k > SLG_MAX_COLLAPSE_ROWS, inner_from + inner_size > SLG_MAX_INNER_HITS with inner hits
// asked for, more than SLG_MAX_SORT_PARTS inner parts (SLG_ERR_UNSUPPORTED).
void check_collapse(const slg_collapse_spec *spec, uint32_t k);
// The checks of a top_hits spec that need no index (slg_batch_prepare_top_hits), against the aggregation spec it
// travels with (null: none; agg_check_spec has passed it).  Throws SlgError: spec NULL, n_nodes == 0, a parent
// that is neither -1 nor a bucket node of aggs, aggs NULL with a child node, a part with an unknown order or a
// negative field other than SLG_SORT_SCORE (SLG_ERR_INVALID, reported first); n_nodes > SLG_MAX_TOP_HITS_NODES,
// size == 0, from + size > SLG_MAX_TOP_HITS, more than SLG_MAX_SORT_PARTS parts, a parent that is itself a child
// (SLG_ERR_UNSUPPORTED).
void check_top_hits(const slg_top_hits_spec *spec, const slg_agg_spec *aggs);

// ---- boolean queries (slg_batch_prepare_bool) ----
// The checks of a bool spec that need no index (throws SlgError): a NULL spec or array, offsets that decrease,
// a c_group that decreases, skips a number or names a group the query does not have, a group without a term,
// an unknown kind, q_min_match > 1 in the batch's score plans (SLG_ERR_INVALID, reported first); more than
// SLG_MAX_BOOL_GROUPS groups or SLG_MAX_BOOL_TERMS clause terms in a query (SLG_ERR_UNSUPPORTED).
void check_bool(const slg_bool_spec *spec, uint32_t nq, const slg_score_plans *plans);
// The clause tables of a checked spec against the segments (slg::BoolQuery / BoolTerm: slg_desc.hpp).
// Throws SLG_ERR_INVALID for a term id out of range.
struct BoolPlan {
  std::vector<slg::BoolQuery> queries;  // [nq]
  std::vector<slg::BoolTerm> terms;     // [total x n_segs], a row per (query, segment)
  uint32_t n_groups = 0;                // groups of the whole batch (0: no query has a clause table)
};
void plan_bool(const std::vector<SegView> &segs, uint32_t nq, const slg_bool_spec &spec, BoolPlan &out);

// ---- nested boolean matchers (slg_batch_prepare_bool_tree) ----
// The checks of a tree spec that need no index (throws SlgError).  SLG_ERR_INVALID, reported first: a NULL spec or
// array, offsets that decrease, check_bool's c_group rules, an unknown kind, a child index that is not below its
// node, a leaf or a node other than the root that no node references, a query with leaves but no node, a negative
// filter id, q_min_match > 1 in the batch's score plans.  SLG_ERR_UNSUPPORTED: more than SLG_MAX_BOOL_TREE_LEAVES
// leaves, SLG_MAX_BOOL_TREE_NODES nodes or SLG_MAX_BOOL_TERMS clause terms in a query, the same child twice in a node.
void check_bool_tree(const slg_bool_tree_spec *spec, uint32_t nq, const slg_score_plans *plans);
// The tables of a checked spec against the segments and the registered filters (slg_desc.hpp: BoolTreeQuery,
// BoolTreeNode, BoolTerm rows, the filter rows and the batch's filter table [row * n_segs + seg]; reject,
// filter_live and n_filters as plan_fscore's).  Throws SLG_ERR_INVALID for a term id out of range or an unknown
// filter id.
struct BoolTreePlan {
  std::vector<slg::BoolTreeQuery> queries;  // [nq]
  std::vector<slg::BoolTreeNode> nodes;     // the nodes of all queries (0: no query has a matcher)
  std::vector<slg::BoolTerm> terms;         // [total x n_segs], a row per (query, segment)
  std::vector<const uint32_t *> filters;    // [filters of the batch x n_segs]
  std::vector<uint32_t> filt_rows;          // the filter leaves of all queries: their rows of `filters`
};
void plan_bool_tree(const std::vector<SegView> &segs, const uint32_t *const *reject, const char *filter_live,
                    size_t n_filters, uint32_t nq, const slg_bool_tree_spec &spec, BoolTreePlan &out);

// ---- phrase queries (slg_index_set_positions, slg_batch_prepare_phrase) ----
// The checks of a segment's positions (throws SlgError): NULL arrays, a first offset other than 0, offsets that
// decrease (SLG_ERR_INVALID); more than 2^32 - 1 positions (SLG_ERR_UNSUPPORTED; from the offsets alone, before a
// position is read); positions that decrease inside a posting, a position >= 2^31 (SLG_ERR_INVALID).
void check_positions(uint64_t n_postings, const uint64_t *pos_offsets, const uint32_t *positions);
// The checks of a phrase spec (and the bool spec beside it, or nullptr) that need no index (throws SlgError).
// SLG_ERR_INVALID, reported first: whatever check_bool refuses in the bool spec, a q_min_should in the bool spec
// (the phrase spec states it), a NULL phrase spec or array, offsets that decrease, a variant without a term, an
// unknown kind, q_min_match > 1 in the batch's score plans.  SLG_ERR_UNSUPPORTED: more than SLG_MAX_PHRASE_TERMS
// terms in a variant, SLG_MAX_PHRASE_VARIANTS variants in a phrase, SLG_MAX_PHRASE_QUERY_TERMS variant terms in
// a query, a slop above SLG_MAX_PHRASE_SLOP, term groups plus phrase groups above SLG_MAX_BOOL_GROUPS.
void check_phrase(const slg_bool_spec *bool_or_null, const slg_phrase_spec *spec, uint32_t nq,
                  const slg_score_plans *plans);
// The tables of a checked pair of specs against the segments (slg_desc.hpp).  bools: plan_bool's tables of the
// term groups, with the phrase groups' bits in the masks and the phrase spec's min_should.  Throws
// SLG_ERR_INVALID for a term id out of range.
struct PhrasePlan {
  BoolPlan bools;
  std::vector<slg::PhraseQuery> queries;  // [nq]
  std::vector<slg::PhraseVar> vars;       // per query, MUST / MUST_NOT / SHOULD groups in that order
  std::vector<slg::PhraseTerm> terms;     // [total x n_segs], a row per (query, segment)
};
void plan_phrase(const std::vector<SegView> &segs, uint32_t nq, const slg_bool_spec *bool_or_null,
                 const slg_phrase_spec &spec, PhrasePlan &out);

// ---- function_score (slg_batch_prepare_fscore) ----
// The checks of a spec that need no index (throws SlgError).  SLG_ERR_INVALID, reported first: a NULL spec or
// array, offsets that decrease, an unknown kind, mode, modifier or decay function, a non-finite weight or factor,
// a non-finite scale or scale <= 0, decay outside (0, 1].  SLG_ERR_UNSUPPORTED: more than SLG_MAX_FSCORE_FUNCS
// functions in a query.
void check_fscore(const slg_fscore_spec *spec, uint32_t nq);
// What plan_fscore sees of a registered aggregation column: per segment its two device arrays, as opaque
// addresses (vals null: the field has no column for that segment)
struct FscoreFieldView {
  int32_t id = 0;
  bool keyword = false, non_finite = false;
  std::vector<slg::ColumnDev> per_seg;     // [n_segs]
  // what only plan_filter_trees reads: the keyword dictionary's size; whether the numeric column was registered
  // from i64 values, the finite minimum and maximum recorded then (when any_value), and whether an i64 value beyond
  // +-2^53 was seen (2^53 + 1 is stored as 2^53: the minimum and maximum alone do not show it)
  uint32_t n_ords = 0;
  bool from_i64 = false, any_value = false, i64_rounded = false;
  double vmin = 0.0, vmax = 0.0;
};
// The lookup of every batch kind that reads a registered aggregation column, in the two steps between which a
// kind checks the field's type.  agg_field: the view of field `id`, or SLG_ERR_INVALID "<before>unknown agg field
// id N<after>".  agg_field_rows: its columns of segments 0 .. n_segs - 1, or SLG_ERR_INVALID "<before>agg field N
// has no column for segment S (added after the field was registered)<after>" for the first segment without one.
const FscoreFieldView &agg_field(const std::vector<FscoreFieldView> &fields, int32_t id, const std::string &before,
                                 const std::string &after);
const slg::ColumnDev *agg_field_rows(const FscoreFieldView &field, uint32_t n_segs, const std::string &before,
                                     const std::string &after);
// The tables of a checked spec against an index state's fields and filters.  reject: the state's flattened
// [filter * n_segs + seg] reject bitmaps (device addresses), filter_live [n_filters] as BatchIn's.  Throws
// SLG_ERR_INVALID for an unknown field or filter id, a keyword column, a field without a column for a segment;
// SLG_ERR_UNSUPPORTED for a column that holds a non-finite value.
struct FscorePlan {
  std::vector<slg::FscoreQuery> queries;   // [nq]
  std::vector<slg::FscoreFn> fns;          // the spec's functions, in its order
  std::vector<slg::ColumnDev> cols;        // [fields the batch names][n_segs]
  std::vector<const uint32_t *> filters;   // [filters the batch names][n_segs]
  uint32_t n_work = 0;                     // queries with work (0: nothing is launched)
  bool full = false;                       // some function needs ln / log1p / log2 / pow
};
void plan_fscore(const std::vector<FscoreFieldView> &fields, const uint32_t *const *reject, const char *filter_live,
                 size_t n_filters, uint32_t n_segs, uint32_t nq, const slg_fscore_spec &spec, FscorePlan &out);

// ---- scan batches (slg_batch_prepare_scan) ----
// The checks of a spec that need no index (throws SlgError).  SLG_ERR_INVALID: a NULL spec or array, an unknown kind
// or modifier, a node filter id below -1, a non-finite q_score of a CONSTANT query, a non-finite q_missing or q_boost
// of a RANK_FEATURE query.  SLG_ERR_UNSUPPORTED, behind those: k > SLG_MAX_K.
void check_scan(const slg_scan_spec *spec, uint32_t nq, uint32_t k);
// The slice tables of a checked spec against an index state's segments, fields and filters: what the selects and
// the aggregation kernels read of any batch (qrefs, slice_seg, the regions' bases in slice_cbeg, cand_total) and
// what scan_kernel reads (queries, slices, cols).  seg_docs: the doc count of every segment; q_filter: the batch's
// root filters or nullptr; full_regions: the batch has a sort spec or aggregations (no query is truncated).
// Throws SLG_ERR_INVALID for an unknown or incomplete filter id (root or node), an unknown field id, a keyword
// column, a field without a column for a segment; SLG_ERR_UNSUPPORTED, behind those, for a column that holds a
// non-finite value.
struct ScanPlan {
  std::vector<slg::ScanQuery> queries;   // [nq]
  std::vector<slg::ScanSlice> slices;    // per query, per segment with docs, ascending first_doc
  std::vector<slg::QueryRef> qrefs;      // [nq]
  std::vector<uint32_t> slice_seg;       // [slices]
  std::vector<uint64_t> slice_cbeg;      // [slices] first entry of the slice's region
  std::vector<slg::ColumnDev> cols;      // [fields the batch names][n_segs]
  std::vector<uint32_t> q_filter;        // [nq] 0 = none, f + 1 (empty when no query has a root filter)
  uint64_t cand_total = 0;               // entries of all regions
  bool full = false;                     // some query needs ln / log1p: the full instantiation
};
void plan_scan(const std::vector<uint32_t> &seg_docs, const std::vector<FscoreFieldView> &fields,
               const char *filter_live, size_t n_filters, uint32_t nq, const slg_scan_spec &spec,
               const int32_t *q_filter, bool full_regions, uint32_t k, ScanPlan &out);

// ---- script_score (slg_batch_prepare_script) ----
// The checks of a spec that need no index (throws SlgError), in ONE walk over each program, which also records the
// static stack positions (ScriptShape).  SLG_ERR_INVALID, reported first: a NULL spec or array, offsets that
// decrease, an unknown op, a const index >= n_consts, a non-finite q_boost.  Behind every invalid argument
// SLG_ERR_UNSUPPORTED: more than SLG_MAX_SCRIPT_INSTRS instructions, a non-finite constant, a stack underflow or a
// final depth other than 1, a stack deeper than SLG_MAX_SCRIPT_DEPTH, more than SLG_MAX_SCRIPT_FIELDS distinct
// fields in a query.  check_script_order: SLG_ERR_INVALID for an order that is neither SLG_SCRIPT_OUTER nor _INNER.
struct ScriptShape {
  std::vector<uint8_t> at;          // per instruction of the spec (from p_offsets[0] on): ScriptInstr's `at`
  std::vector<uint32_t> max_depth;  // [nq] the deepest stack of each program (0: no program)
  uint32_t batch_max_depth = 0;
};
void check_script(const slg_script_spec *spec, uint32_t nq, ScriptShape &shape);
void check_script_order(int order);
// The tables of a checked spec against an index state's fields.  Throws SLG_ERR_INVALID for an unknown field id,
// a keyword column, a field without a column for a segment; behind those SLG_ERR_UNSUPPORTED for a column that
// holds a non-finite value.
struct ScriptPlan {
  std::vector<slg::ScriptQuery> queries;  // [nq]
  std::vector<slg::ScriptInstr> instrs;   // the spec's instructions, in its order
  std::vector<slg::ColumnDev> cols;       // [fields the batch names][n_segs]
  uint32_t n_work = 0;                    // queries with a program (0: nothing is launched)
  uint32_t max_depth = 0;                 // the deepest stack of the batch's programs
};
void plan_script(const std::vector<FscoreFieldView> &fields, uint32_t n_segs, uint32_t nq, const slg_script_spec &spec,
                 const ScriptShape &shape, ScriptPlan &out);

// ---- filter trees (slg_index_add_filter_trees) ----
// The checks of the trees that need no index (throws SlgError).  SLG_ERR_INVALID, reported first: NULL arrays,
// n_trees == 0, n_nodes == 0, an unknown kind, a program that underflows the stack or does not end with exactly
// one value, an arity larger than the stack, a NaN bound, ord_begin + n_ords_in > n_ords.  Then
// SLG_ERR_UNSUPPORTED: more than SLG_MAX_FILTER_NODES nodes, a stack deeper than SLG_MAX_FILTER_DEPTH, more than
// SLG_MAX_FILTER_TREES trees.
void check_filter_trees(const slg_filter_tree *trees, uint32_t n_trees);
// The device image of checked trees against an index state's fields and filters (reject, filter_live, n_filters
// as plan_fscore's; a filter without a bitmap for some segment has nullptr there).  Throws SLG_ERR_INVALID for an
// unknown field or filter id, a field or filter without data for every segment, the wrong column kind, an ordinal
// >= the field's n_ords; behind those SLG_ERR_UNSUPPORTED for an i64 column beyond +-2^53.
struct FilterTreePlan {
  std::vector<slg::FilterTreeDev> trees;   // [n_trees]
  std::vector<slg::FilterNodeDev> nodes;   // every tree's nodes, in its order
  std::vector<slg::ColumnDev> cols;        // [fields the trees name][n_segs]
  std::vector<const uint32_t *> filters;   // [filters the trees name][n_segs]
  std::vector<uint32_t> words;             // one bit set of ceil(n_ords / 32) words per KEYWORD_IN node
};
void plan_filter_trees(const std::vector<FscoreFieldView> &fields, const uint32_t *const *reject,
                       const char *filter_live, size_t n_filters, uint32_t n_segs, const slg_filter_tree *trees,
                       uint32_t n_trees, FilterTreePlan &out);

// ---- nested filter trees (slg_index_add_nested_filter_trees) ----
// The checks of the trees that need no index (throws SlgError), in the order the header gives: SLG_ERR_INVALID
// first (what check_filter_trees refuses in each scope's program, and the scope list itself), then
// SLG_ERR_UNSUPPORTED for the limits.
void check_nested_filter_trees(const slg_nested_filter_tree *trees, uint32_t n_trees);
// What the planner sees of a registered nested path / nested value column: per segment its device arrays as
// opaque addresses (a path without tables for a segment: base null; a column: has[s] == 0)
struct NestedPathView {
  int32_t id = 0, parent = -1;
  std::vector<slg::NestedPathDev> per_seg;  // [n_segs]
};
struct NestedFieldView {
  int32_t id = 0, path = 0;
  int kind = 0;  // 1 f64, 2 i64, 3 keyword ordinals
  uint32_t n_ords = 0;
  std::vector<slg::NestedColDev> per_seg;  // [n_segs]
  std::vector<char> has;                   // [n_segs] (a column's doc_offs may be null: no value in that segment)
};
// The device image of checked trees against an index state (fields, reject, filter_live, n_filters as
// plan_filter_trees', whose doc-level leaves these trees share).  The scope rows are ordered by level: object
// scopes of level l (l = 1: no NESTED leaf) are rows level_begin[l - 1] .. level_begin[l]; the doc-level scopes
// follow from level_begin.back() on, in tree order.  Throws SLG_ERR_INVALID for an unknown id, data missing for a
// segment, the wrong column kind, an ordinal out of range, a NESTED leaf of an object scope whose child path is
// not registered under the scope's path; behind those SLG_ERR_UNSUPPORTED for the doc level's 2^53 rule.
struct NestedFilterPlan {
  std::vector<slg::NestedScopeDev> scopes;
  std::vector<uint32_t> level_begin;        // [levels + 1]
  std::vector<slg::FilterNodeDev> nodes;    // every scope's nodes, in row order
  std::vector<slg::ColumnDev> cols;         // [agg fields the trees name][n_segs]
  std::vector<const uint32_t *> filters;    // [filters the trees name][n_segs]
  std::vector<uint32_t> words;              // the ordinal bit sets
  std::vector<slg::NestedPathDev> paths;    // [paths the trees name][n_segs]
  std::vector<slg::NestedColDev> ncols;     // [nested fields the trees name][n_segs]
};
void plan_nested_filter_trees(const std::vector<FscoreFieldView> &fields, const uint32_t *const *reject,
                              const char *filter_live, size_t n_filters, const std::vector<NestedPathView> &paths,
                              const std::vector<NestedFieldView> &nested_fields, uint32_t n_segs,
                              const slg_nested_filter_tree *trees, uint32_t n_trees, NestedFilterPlan &out);

// Throws SlgError (SLG_ERR_INVALID / SLG_ERR_UNSUPPORTED) on malformed input.
void plan_batch(const std::vector<SegView> &segs, const slg_tuning &tune, const BatchIn &in, Plan &out);

}  // namespace slgplan
