// slg_desc.hpp — the descriptors a query batch is planned into (host) and consumed from (device),
// and the constants both sides share.  Plain C++: included by the HIP translation units through
// slg_wave.hpp and by the host-only planner (slg_plan.cpp, built with g++ for the CPU unit tests).
#pragma once

#include <stdint.h>
#include <climits>

#if defined(__HIPCC__)
#define SLG_HD __host__ __device__
#else
#define SLG_HD
#endif

namespace slg {

constexpr uint32_t kEmptyKey = 0xFFFFFFFFu;
constexpr uint32_t kDocEnd = 0xFFFFFFFFu;
constexpr int32_t kSentinelTk = INT32_MIN;
constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr uint32_t kMaxTerms = 32;
constexpr int kChampSorted = 64;  // exact-rank lower bounds (sorted lane maxima)
constexpr int kChampions = 68;    // + bounds for ranks 128, 256, 512, 1024
// LDS bytes of the buffered top-k of a scoring wave (BufTopK<KREGS>::kEntries 64-bit keys)
constexpr int buftopk_lds(int kregs) { return 64 * (kregs + 1) * 8; }
// index of the champion entry that bounds the k-th largest impact of a term from below
SLG_HD inline int champ_index(uint32_t k) {
  return k <= 64 ? (int)k - 1 : k <= 128 ? 64 : k <= 256 ? 65 : k <= 512 ? 66 : 67;
}

// ---- device-side descriptors (built on the host per batch) ---------------------------
// Posting arrays are PADDED per list: list t starts at term_offsets[t] + kListPad * t and is
// followed by kListPad sentinel entries (doc = kDocEnd, impact = 0), so a whole 64-lane slot
// loaded at ANY posting of a list never reads another list's postings: lanes past the list's end
// see sentinels, lanes past a round's cut see later postings of the same list (docs >= the round's
// end).  The scoring kernels therefore need no per-slot lane count to tell real postings from
// foreign ones.  null_idx = a 64-entry run of sentinels (the slot unused descriptor lanes load).
constexpr uint32_t kListPad = 64;
constexpr uint32_t kNullRun = 576;  // sentinels at null_idx: a whole round of idle lanes (64 x 8) + a slot
struct SegDev {
  const uint32_t *docs;     // [P + kListPad * V + kNullRun] doc ids
  const float *imps;        // same layout: precomputed bm25 (weight == 1) per posting
  const uint32_t *deleted;  // bitmap words or nullptr
  const float *champ;       // [V * kChampions] per-term descending impact lower bounds
  uint32_t n_docs;
  uint32_t pad;
  uint64_t null_idx;        // index of kNullRun sentinel entries
};

struct TermRef {  // one scored term of one sub-query
  uint64_t off;   // posting offset inside the segment arrays
  uint32_t df;    // list length
  float weight;
  uint32_t term;  // term id inside the segment (champion table row)
  uint32_t leaf;  // ScorePlan leaf the term's scores add to (non-decreasing inside a sub-query)
  // two-level plans (RoundQuery::n_groups != 0): the group of the leaf = bits 0..7, leaves the plan
  // gives that group (present in this segment or not) = bits 8..15, bit 16 = the group is a DisMax
  uint32_t gmeta;
  float gtie;     // the group's tie breaker
};

struct RoundQuery {  // sub-query = (query, segment) pair with >= 1 non-empty term
  uint32_t q, seg;
  uint32_t term_begin, n_terms;
  uint32_t slice_begin, n_slices;
  uint32_t n_rounds;      // doc-range rounds of <= ~kRoundTarget postings
  uint32_t rounds_per_slice;
  uint32_t bounds_begin;  // bounds[bounds_begin + j*n_terms + t], j = 0..n_rounds
  uint32_t rdoc_begin;    // rdoc[rdoc_begin + j]: first doc id of round j (j = n_rounds: end)
  uint32_t bnd_begin;     // first boundary task of this sub-query (partition kernel)
  uint32_t longest;       // index of the longest ESSENTIAL list (splitter source)
  uint32_t ess_mask;      // bit t: list t is essential (MaxScore); the others are only probed
  uint32_t skip_mask;     // bit t: non-essential list t is sparse-probed: its 64-posting blocks are
                          // tested against the candidate docs before they are loaded (block skipping)
  uint32_t filter;        // 0: none; f + 1: docs must also pass filter f (reject table row f)
  uint32_t cand_lo, cand_hi;  // large-k mode: first candidate slot of this sub-query (u64)
  // score plan (query/planner.rs:113-153): 0 = every term its own leaf, summed (the flat sum in
  // term order); 1 = Sum of leaves that group several terms; 2 = DisMax of leaves
  uint32_t plan;
  float tie;       // DisMax tie breaker
  float max_init;  // DisMax: 0.0 if some leaf of the plan has no term in this segment, else -inf
  uint32_t n_leaves;  // leaves of the plan (a DisMax counts every one, absent ones as 0.0)
  uint32_t n_groups;  // two-level plan: the root combines this many groups of leaves (0: flat plan)
  // threshold seed (0: none): theta0 = max_t w_t * champ[t][rank(k)].  At least k live docs have
  // a single contribution >= theta0 and a doc's total is >= any one of its non-negative
  // contributions (Sum, or DisMax with tie in [0, 1]), so nothing below theta0 reaches the top-k.
  // Set by the host planner from its mirror of the champion table; never with a doc filter (it
  // may reject the champions) or a negative weight.
  float theta0;
  // deep score trees (slg_score_plans::q_node_offsets, > 2 levels): depth = levels of Sum / DisMax nodes
  // above the leaves (0: not a deep tree), node_begin = the query's first PlanNode in the image
  uint32_t depth, node_begin;
};

// One Sum / DisMax node of a deep score tree, in the CANONICAL form the planner builds: every leaf hangs
// at the same depth (a leaf higher up gets a chain of one-child Sum nodes: Sum of one child is the
// child, bit for bit), so level l of the tree = the nodes at distance l from the root.  TermRef::gmeta
// of a term = the node its leaf hangs off (level depth - 1).
constexpr uint32_t kMaxPlanDepth = 4;  // = SLG_MAX_PLAN_DEPTH (searchlite_gpu.h; checked in slg_plan.cpp)
struct PlanNode {
  uint32_t parent;      // node index inside the query's table (the root: itself)
  uint32_t n_children;  // children the plan gives the node (present in this segment or not)
  uint32_t kind;        // 0 Sum, 1 DisMax
  float tie;
};

// What a scoring wave needs to start its slice, gathered in one record per launch position by
// partition_rounds_kernel (a wave then starts with ONE dependent load instead of a chain of four).
struct SliceDesc {
  uint32_t slice;       // slice index (candidate output arrays)
  uint32_t term_begin;  // first TermRef of the sub-query
  uint32_t bounds_off;  // bounds[] index of the slice's first cut points
  uint32_t rdoc_off;    // rdoc[] index of the slice's first round
  uint32_t n_terms, n_rounds, seg, filter;
  uint32_t q;
  float theta0;
  uint32_t cand_lo, cand_hi;
  // for waves that cut their slice themselves (slg_score_uni4.hpp with RoundScoreParams::bounds ==
  // nullptr): the slice's first round, the sub-query's rounds, its splitter list
  uint32_t first_round, sq_rounds, longest;
  uint32_t l_df;   // the splitter list's length and posting offset: its stride positions are read
  uint64_t l_off;  // straight off this record, beside the TermRef loads instead of behind them
  // score plan of the sub-query (RoundQuery::plan / tie / max_init / n_leaves), for the few-term
  // kernel's plan instantiation (flat plans: Sum or DisMax over leaves of one or more terms)
  uint32_t plan;
  float tie, max_init;
  uint32_t n_leaves;
};

struct QueryRef {
  uint32_t slice_begin, slice_end;  // all slices of all sub-queries of this query
};


// ---- vector stores (slg_rerank.hpp, slg_vsearch.hpp) ----------------------------------------------
// A segment without vectors in the field has dim 0 and the field's metric.  A candidate whose segment
// is >= n_segs, or whose doc is >= its segment's n_docs, is a candidate without a vector: it scores
// missing_vector_score of the field's metric (api/reader.rs:217-223).
struct VecSegDev {
  const uint32_t *offsets;  // [n_docs] row index or 0xFFFFFFFF
  const float *values;      // [rows * dim]
  uint32_t n_docs;
  uint32_t dim;
  int32_t metric;  // 0 cosine, 1 l2
  uint32_t pad;
};
// The bf16 copy of a segment's store (slg_index_quantize_vector_field; slg_vsearch_approx.hpp): the rows of
// VecSegDev::values in the same order, rounded to nearest even, each padded with zeros to dim_pad values, and
// the f32 squared norm of each f32 row.  rows == nullptr: the segment has no vectors in the field.
struct VecCopyDev {
  const uint16_t *rows;  // [rows * dim_pad] bf16 bit patterns
  const float *norms;    // [rows]
  uint32_t dim_pad;
  uint32_t pad;
};
// The inverted-file lists of a segment's store (slg_index_cluster_vector_field; slg_vsearch_ivf.hpp): list l holds
// docs[list_begin[l] .. list_begin[l + 1]), ascending.  list_begin == nullptr: the segment is unclustered.
struct VecListDev {
  const uint32_t *list_begin;  // [n_lists + 1]
  const uint32_t *docs;
  uint32_t n_lists;
  uint32_t pad;
};
// an unclustered segment with vectors in a clustered field: every query scans it whole, as a list behind the field's own
constexpr uint32_t kIvfUnclChunks = 32;  // doc chunks of an unclustered segment, at most
struct IvfUncl {
  uint32_t seg, n_docs;
  uint32_t chunk_docs;  // docs of a chunk (a multiple of the scan tile's 128)
  uint32_t slot;        // the first of its partial slots among the unclustered segments' (one per chunk)
};

// ---- query rescore (slg_batch_prepare_rescore; kernel: slg_rescore.hpp, planner: slg_plan.cpp) -------
// The rescore terms of query q are terms[(term_begin + i) * n_segs + s], i = 0 .. n_terms - 1, for
// segment s: sorted by leaf (stable, so a leaf's terms keep the query's term order); a term absent
// from a segment (SLG_NO_TERM or an empty list) has df 0.
struct RescoreTerm {
  uint64_t off;  // posting offset inside the segment arrays (padded layout, as TermRef::off)
  uint32_t df;   // list length; 0: the segment has no posting of the term
  float weight;
  uint32_t leaf;
  uint32_t pad;
};
struct RescoreQuery {
  uint32_t term_begin, n_terms;
  uint32_t window;     // rows offered to the rescore (the kernel caps it at the query's row count)
  uint32_t mode;       // SLG_RESCORE_*
  uint32_t plan;       // 0 Sum, 1 DisMax over the leaves
  float tie;
  uint32_t n_leaves;   // leaves of the plan (a DisMax counts every one, those without a posting as 0.0)
  uint32_t min_match;  // leaves that must hold a row's doc (already >= 1)
};
constexpr uint32_t kRescoreMaxWindow = 1024;  // = SLG_MAX_RESCORE_WINDOW: the widest WaveTopK
constexpr uint32_t kRescoreMaxTable = 2048;   // RescoreTerm entries of one query (terms x segments) in LDS: 48 KB

// ---- boolean queries (slg_batch_prepare_bool; kernel: slg_bool.hpp, planner: slg_plan.cpp) -----------
// The clause terms of query q in segment s are terms[term_begin * n_segs + s * n_terms + i], i = 0 ..
// n_terms - 1: one contiguous row per (query, segment), which is what a wave of bool_filter_kernel reads.
// Inside a row the terms lie MUST first, MUST_NOT second, SHOULD last (stable: a kind's terms keep the
// caller's order), so the kernel's early outs see the clauses that reject first; a term absent from a
// segment (SLG_NO_TERM or an empty list) has df 0.
struct BoolTerm {
  uint64_t off;    // posting offset inside the segment arrays (padded layout, as TermRef::off)
  uint32_t df;     // list length; 0: the segment has no posting of the term
  uint32_t group;  // the term's group inside its query (< kBoolMaxGroups: a bit of the masks)
};
struct BoolQuery {
  uint32_t term_begin, n_terms;  // n_terms 0: the query has no clause table and is left as it is
  uint32_t must_mask, must_not_mask, should_mask;  // bit g: group g is of that kind
  uint32_t min_should;
  uint32_t n_must, n_must_not;   // terms of MUST groups (the row's first), of MUST_NOT groups (behind them)
};
constexpr uint32_t kBoolMaxGroups = 32;  // = SLG_MAX_BOOL_GROUPS
constexpr uint32_t kBoolMaxTerms = 64;   // = SLG_MAX_BOOL_TERMS

// ---- nested boolean matchers (slg_batch_prepare_bool_tree; kernel: slg_booltree.hpp, planner: slg_plan.cpp) ----
// One candidate's state is a pair of 64-bit masks over the query's VALUES: bit l < 32 is leaf l (the term groups,
// then the filter leaves), bit 32 + i is node i.  The nodes of query q are nodes[node_begin .. node_begin +
// n_nodes) in post-order (a node child lies below its parent), the last one the root.  The clause terms are
// BoolTerm rows as above, one per (query, segment); BoolTerm::group holds the term's leaf in bits 0-4 and
// kBoolTreeLeafEnd where the term is the last of its leaf.  Inside a row the terms of the leaves that reach the
// root over MUST / MUST_NOT edges only come first (they alone can reject on their own), then the others, each
// class in the caller's order, a leaf's terms side by side.  Filter leaf i of the query (leaf n_leaves -
// n_filters + i) passes where filters[filt_rows[filt_begin + i] * n_segs + seg] has the doc's bit clear or is null.
struct BoolTreeQuery {
  uint32_t term_begin, n_terms;
  uint32_t node_begin, n_nodes;  // n_nodes 0: the query has no matcher and is left as it is
  uint32_t n_leaves;             // term groups + filter leaves
  uint32_t filt_begin, n_filters;
  uint32_t pad;
};
struct BoolTreeNode {
  uint64_t must, must_not, should;  // the node's children of each kind, as value bits
  uint32_t min_should;
  uint32_t pad;
};
constexpr uint32_t kBoolTreeMaxLeaves = 32;   // = SLG_MAX_BOOL_TREE_LEAVES
constexpr uint32_t kBoolTreeMaxNodes = 32;    // = SLG_MAX_BOOL_TREE_NODES
constexpr uint32_t kBoolTreeLeafEnd = 0x100;  // in BoolTerm::group: the last term of its leaf

// The three-valued pass over a query's nodes.  t: the values known to be true, f: the values known to be false
// (disjoint; a value in neither is open).  Walks the nodes in order — children first — and puts every node that
// is decided by what is known into t or f.  node_at(i) -> BoolTreeNode i of the query.
//   sure true:  every MUST child true, every MUST_NOT child false, at least min_should SHOULD children true;
//   sure false: a MUST child false, a MUST_NOT child true, or fewer than min_should SHOULD children not false.
// Sound because a node's value is MONOTONE in what is known: learning an open value moves bits INTO t or f and
// never out, (t & must) == must and popc(t & should) only grow with t, popc(should & ~f) only shrinks with f —
// so a node that is sure stays sure, and equals its value under every completion of the open leaves.  With every
// leaf known every node is decided (by induction over the order: all of a node's children are in t | f, so
// either all three tests of `sure true` hold or one of `sure false` does).
template <typename NodeAt>
SLG_HD inline void booltree_eval(NodeAt node_at, uint32_t n_nodes, uint64_t &t, uint64_t &f) {
  for (uint32_t i = 0; i < n_nodes; i++) {
    const BoolTreeNode n = node_at(i);
    const bool yes = (t & n.must) == n.must && (f & n.must_not) == n.must_not &&
                     (uint32_t)__builtin_popcountll(t & n.should) >= n.min_should;
    const bool no = (f & n.must) != 0ull || (t & n.must_not) != 0ull ||
                    (uint32_t)__builtin_popcountll(n.should & ~f) < n.min_should;
    const uint64_t bit = 1ull << (32u + i);
    if (yes) t |= bit;
    if (no) f |= bit;
  }
}

// ---- phrase queries (slg_batch_prepare_phrase; kernel: slg_phrase.hpp, planner: slg_plan.cpp) --------
// A phrase batch carries the bool tables above for its term groups (BoolQuery's masks and min_should cover
// the phrase groups too: they are numbered behind the query's term groups) and three tables of its own.
// The variants of query q are vars[var_begin .. var_begin + n_vars), the same for every segment, ordered
// MUST groups first, MUST_NOT second, SHOULD last (stable) with a group's variants side by side.  The
// variant terms of query q in segment s are pterms[term_begin * n_segs + s * n_terms + i]: one contiguous
// row per (query, segment) in the spec's order; a variant's terms are row[t_begin .. t_begin + n).  A
// variant that is DROPPED in a segment (a term absent or with df 0 there, or the segment has no positions)
// has df 0 in every one of its terms of that segment's row, so its first term tells.
struct PosSegDev {          // per segment of an index state (slg_index_set_positions)
  const uint32_t *offs;     // [P + 1] first position of each posting, in the UNPADDED posting order; or nullptr
  const uint32_t *pos;      // [offs[P]] positions, non-decreasing inside a posting
};
struct ExpandSegDev {           // per segment of an index state (slg_index_set_terms): its dictionary in byte order
  const unsigned char *bytes;   // the sorted keys back to back; or nullptr
  const uint32_t *offs;         // [n + 1]
  const uint8_t *nchars;        // [n] chars of each key; 255: 255 or more
};
struct SuggestSegDev {          // the same dictionary as slg_suggest_batch reads it: with the keys' doc frequencies
  const unsigned char *bytes;   // (ExpandSegDev's three arrays; nullptr without a dictionary)
  const uint32_t *offs;
  const uint8_t *nchars;
  const uint32_t *df;           // [n] posting-list length of the key at each sorted position, as staged
};
struct TextSegDev {             // per segment of a text field (slg_index_add_text_field): its docs' texts
  const uint8_t *bytes;         // the texts back to back, 16-byte aligned and padded by 16 bytes; or nullptr
  const uint64_t *offs;         // [n_docs + 1]
  const uint32_t *non_ascii;    // bit d: doc d's text holds a byte >= 0x80
  uint32_t n_docs;
  uint32_t pad_;
};
struct PhraseTerm {
  uint64_t off;    // posting offset inside the segment arrays (padded layout, as BoolTerm::off)
  uint64_t ubase;  // the list's first posting in the unpadded order (= term_offsets[term]): PosSegDev::offs index
  uint32_t df;     // list length; 0: the variant is dropped in this segment
  uint32_t pad;
};
struct PhraseVar {
  uint32_t t_begin;  // first term of the variant inside the (query, segment) row
  uint32_t n_last;   // bits 0-7: terms (1 .. kPhraseMaxTerms); bit 8: the last variant of its group
  uint32_t group;    // the phrase's group inside its query (a bit of BoolQuery's masks)
  uint32_t slop;
};
struct PhraseQuery {
  uint32_t var_begin, n_vars;
  uint32_t term_begin, n_terms;
  uint32_t n_term_groups;  // groups 0 .. n_term_groups - 1 are term groups (BoolTerm rows), the rest phrases
  uint32_t pad[3];
};
constexpr uint32_t kPhraseMaxTerms = 8;        // = SLG_MAX_PHRASE_TERMS (the kernel's unrolled cursors)
constexpr uint32_t kPhraseMaxVariants = 8;     // = SLG_MAX_PHRASE_VARIANTS
constexpr uint32_t kPhraseMaxQueryTerms = 64;  // = SLG_MAX_PHRASE_QUERY_TERMS
constexpr uint32_t kPhraseMaxSlop = 0x7FFFFFFFu - kPhraseMaxTerms;  // = SLG_MAX_PHRASE_SLOP
constexpr uint32_t kPositionEnd = 0x80000000u;  // positions are below it (the reference's gaps are i32)

// ---- registered columns of one segment, as every batch kind's tables hold them ------------------------
// (the device code that reads them: slg_wave.hpp column_range, sorted_key)
// An aggregation column (slg_index_add_agg_field_*): aggregations, function_score, filter trees, collapse
struct ColumnDev {
  const uint32_t *offs;  // [n_docs + 1] into vals, or nullptr: every doc has exactly one value, vals[doc]
  const void *vals;      // double[] (numeric) or uint32_t[] (keyword ordinals); nullptr: the segment has no column
  SLG_HD const double *f64() const { return static_cast<const double *>(vals); }
  SLG_HD const uint32_t *ords() const { return static_cast<const uint32_t *>(vals); }
};
// One part of a sort (slg_index_add_sort_field_*): the sorted select, the inner sort of collapse
struct SortColDev {
  const unsigned long long *key;  // [n_docs] u64 key of the part's order (0 for Missing docs)
  const uint32_t *present;        // presence bitmap (bit d & 31 of word d >> 5)
};
constexpr uint32_t kSortMaxParts = 4;  // SLG_MAX_SORT_PARTS
constexpr uint32_t kSortWords = 3 * kSortMaxParts + 2;  // of a sort key: three per part, segment, doc

// ---- function_score (slg_batch_prepare_fscore; kernel: slg_fscore.hpp, planner: slg_plan.cpp) --------
// The functions of query q are fns[fn_begin .. fn_begin + n_fns), in request order, the same for every segment.
// A function's column is cols[col * n_segs + seg], its filter's reject bitmap filters[(filter - 1) * n_segs + seg].
struct FscoreQuery {
  uint32_t fn_begin, n_fns;
  uint32_t modes;      // bits 0-7 score mode, 8-15 boost mode, 16-23 SLG_FSCORE_HAS_* flags
  uint32_t work;       // 0: no function, no max_boost, no min_score, boost 1 — the query is left as it is
  float max_boost, min_score, boost;
  uint32_t pad;
};
struct FscoreFn {
  uint32_t kinds;      // bits 0-7 SLG_FSCORE_* kind, 8-15 modifier, 16-23 decay function
  uint32_t col;        // the function's row of the column table (weight: unused)
  uint32_t filter;     // 0: none; r + 1: row r of the batch's filter table
  float weight;        // weight, or field_value_factor's factor
  double missing, origin, scale, offset, decay;
  int32_t field;       // the agg field id the caller named, -1 for a weight (what an explanation reports; no kernel
                       // between scoring and select reads it)
  uint32_t pad;
};
constexpr uint32_t kFscoreMaxFuncs = 8;  // = SLG_MAX_FSCORE_FUNCS

// ---- script_score (slg_batch_prepare_script; kernel: slg_script.hpp, planner: slg_plan.cpp) --------
// The program of query q is instrs[instr_begin .. instr_begin + n_instrs), in reverse Polish order, the same for
// every segment.  The stack positions of such a program are static: the planner records with every instruction
// the slot it works at, and the kernel never tracks a stack pointer.  The query's distinct fields are numbered in
// order of first use; field f's column is cols[col[f] * n_segs + seg].
constexpr uint32_t kScriptMaxInstrs = 64, kScriptMaxDepth = 8, kScriptMaxFields = 8;  // = SLG_MAX_SCRIPT_*
struct ScriptQuery {
  uint32_t instr_begin, n_instrs;   // n_instrs 0: the query is left as it is
  uint32_t n_fields;
  float boost;
  uint32_t max_depth;               // the deepest stack of the program
  uint32_t pad[3];
  uint32_t col[kScriptMaxFields];   // the fields' rows of the column table
};
struct ScriptInstr {
  uint32_t code;   // bits 0-7 SLG_SCRIPT_* op; 8-15 `at`: the slot the result is written to — a push: the depth
                   // before it; ADD / SUB / MUL / DIV: a = slot at, b = slot at + 1; NEG: slot at; 16-23 PUSH_FIELD:
                   // the field's number in the query
  uint32_t pad;
  double value;    // PUSH_CONST
};

// ---- filter trees (slg_index_add_filter_trees; kernel: slg_filter.hpp, planner: slg_plan.cpp) --------
// The image of one call: trees[n_trees], nodes (every tree's, in postfix order), the column table, the filter
// table, the words of the ordinal bit sets.  A leaf's column is cols[row * n_segs + seg] (ColumnDev; a keyword
// column's vals are u32 ordinals), a FILTER_ID leaf's reject bitmap filters[row * n_segs + seg].
struct FilterTreeDev {
  uint32_t node_begin, n_nodes;
};
struct FilterNodeDev {
  uint32_t kind;   // SLG_FILTER_*
  uint32_t arity;  // AND / OR
  uint32_t row;    // a leaf's row of the column table, or of the filter table (FILTER_ID)
  uint32_t bits;   // KEYWORD_IN: first word of the node's ordinal bit set (ceil(n_ords / 32) words)
  double lo, hi;   // RANGE_F64 as given; RANGE_I64 clamped into +-2^53 (or the infinity: nothing passes)
};
constexpr uint32_t kFilterMaxNodes = 64, kFilterMaxDepth = 16, kFilterMaxTrees = 64;  // = SLG_MAX_FILTER_*
constexpr uint32_t kFilterKeywordIn = 0, kFilterRangeF64 = 1, kFilterRangeI64 = 2, kFilterId = 3, kFilterAnd = 4,
                   kFilterOr = 5, kFilterNot = 6;

// ---- nested filter trees (slg_index_add_nested_filter_trees; kernel: slg_nested.hpp, planner: slg_plan.cpp) ----
// The image of one call grows the one above by scope rows and two tables.  A tree is a list of scopes: object
// scopes (a postfix program evaluated per OBJECT of the scope's path) and, last, the doc-level scope.  The rows
// are ordered by level: every tree's object scopes without a NESTED leaf first, then those one level up, ...,
// then the doc-level scopes in tree order; a level is one launch per segment.  A NESTED leaf's `row` is the scope
// row of its child; object scope r writes the pass bits of its objects to obj_bits[r * n_segs + seg].  In an
// object scope a leaf's `row` is a row of the nested column table, RANGE_I64 keeps its bounds as int64 in the
// bits of lo / hi, and a leaf that can pass nothing (a field of another path) is OR of nothing.
struct NestedScopeDev {
  uint32_t node_begin, n_nodes;
  uint32_t path_row;  // the scope's row of the path table (doc level: unused)
  uint32_t pad;
};
struct NestedPathDev {     // one registered path in one segment
  const uint32_t *base;      // [n_docs + 1] first object of each doc (the prefix sum of the counts)
  const uint32_t *obj_doc;   // [n_objects] the doc of each object
  const uint32_t *par_offs;  // [n_docs + 1] into parents, or nullptr: no object binds to a parent
  const uint32_t *parents;   // the parent object's index within the doc (0xFFFFFFFF: none)
  uint32_t n_objects, pad;
};
struct NestedColDev {      // one registered nested value column in one segment
  const uint32_t *doc_offs;  // [n_docs + 1] first object of each doc, or nullptr: the segment has no value
  const uint32_t *obj_offs;  // [objects + 1] into vals (a doc may have fewer objects here than its path counts)
  const void *vals;          // double[], int64_t[] or uint32_t[] (keyword ordinals)
};
constexpr uint32_t kFilterNested = 7;
constexpr uint32_t kNestedMaxScopes = 16, kNestedMaxDepth = 4;  // = SLG_MAX_NESTED_*

// ---- scan batches (slg_batch_prepare_scan; kernel: slg_scan.hpp, planner: slg_plan.cpp) --------------
// A query without a scored term has no posting list: its candidates are the docs of every segment that pass the
// bitmaps.  A (query, segment) pair is cut into slices of kScanSliceDocs consecutive docs — a multiple of 2048, so
// that a slice starts at a bitmap word and a wave's step of 64 words never straddles two slices.  A slice's region
// of the candidate buffer starts at slice_cbeg[s] and holds `cap` entries: the slice's doc count (full form), or
// min(doc count, k) (truncated form: every score of the query is equal, no sort, no aggregation — the first k
// passing docs of a slice are the only ones the select can take from it; the rest are counted, not stored).
#ifndef SLG_SCAN_SLICE_DOCS
#define SLG_SCAN_SLICE_DOCS 16384
#endif
constexpr uint32_t kScanSliceDocs = SLG_SCAN_SLICE_DOCS;
static_assert(kScanSliceDocs % 2048 == 0 && kScanSliceDocs != 0, "64 lanes x one bitmap word");
constexpr uint32_t kScanMatchAll = 0, kScanConstant = 1, kScanRankFeature = 2;  // = SLG_SCAN_*
constexpr uint32_t kScanModNone = 0, kScanModLog = 1, kScanModLog1p = 2, kScanModSqrt = 3, kScanModReciprocal = 4;
struct ScanQuery {
  uint32_t kind;      // SLG_SCAN_*
  uint32_t modifier;  // SLG_SCAN_MOD_* (rank_feature)
  uint32_t filter;    // the node's own filter: 0 none, f + 1 (a row of the state's reject table)
  uint32_t col;       // rank_feature: the field's row of the batch's column table
  float score;        // constant_score: boost * node_boost (match_all: 1.0)
  float missing;      // rank_feature: the value of a doc without one
  float boost;        // rank_feature
  uint32_t pad;
};
struct ScanSlice {
  uint32_t q, seg;
  uint32_t first_doc;  // a multiple of kScanSliceDocs
  uint32_t n_docs;     // 1 .. kScanSliceDocs
  uint32_t cap;        // entries of the slice's region (n_docs, or min(n_docs, k) in the truncated form)
  uint32_t pad[3];
};

// ---- merge of per-shard results gathered over RCCL (merge_shards_kernel, slg_kernels.hpp) ----------
struct ShardMergeParams {
  const uint32_t *doc;    // shard sh's rows start at doc + sh * arr_stride ([nq*k] each)
  const uint32_t *seg;
  const float *score;
  const uint32_t *count;  // shard sh's counts start at count + sh * cnt_stride ([nq])
  uint32_t *out_doc, *out_seg;
  float *out_score;
  uint32_t *out_count;
  uint32_t n_shards, nq, k, seg_stride;
  // elements between two shards' arrays: nq*k / nq for separate shard-major arrays; (3k+1)*nq for
  // both when the shards' contiguous result blocks doc|seg|score|count lie one after another, as an
  // all-gather delivers them
  uint64_t arr_stride, cnt_stride;
};

// ---- planning constants (the kernels that consume them: slg_score*.hpp) ------------------------
constexpr int kMaxRoundsPerSlice = 16;  // and (rounds+1)*T <= 64: cut points live in one VGPR
constexpr int kDefaultRoundsPerSlice = 8;
#ifndef SLG_UNI_RPS
#define SLG_UNI_RPS 4
#endif
constexpr int kUniRoundsPerSlice = SLG_UNI_RPS;  // few-term kernel, k <= 64
constexpr int kSpanWords = 512;           // bitmap words per window (many-term kernel)
constexpr uint32_t kSpan = kSpanWords * 32;  // docs per window
constexpr int kUniSlots = 8;                 // 64-posting slots per round
constexpr int kUniCap = kUniSlots * 64;      // postings per round
constexpr int kUniMaxLists = 4;              // lists per sub-query on the few-term kernel's 4-bit-field form
constexpr int kU4MaxLists = 8;               // lists per sub-query on the few-term kernel (8-bit fields)
constexpr int kMultiCap = 512;       // accumulators (= distinct docs) per chunk
constexpr int kMultiTarget = 448;    // planned postings per round (host; measured optimum 448-480)

}  // namespace slg
