"""ctypes binding of include/searchlite_gpu.h.

There is no fallback: if libsearchlite_gpu.so is missing the import of anything that needs
it raises, and every call either runs the HIP kernels or raises SlgError.
"""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

NO_TERM = 0xFFFFFFFF
NO_VECTOR = 0xFFFFFFFF
MAX_QUERY_TERMS = 32
MAX_K = 20001
MAX_RERANK_K = 1024
MAX_VECTOR_CLAUSES = 8
MAX_VECTOR_CANDIDATES = 10000
MAX_VECTOR_LISTS = 65536
MAX_VECTOR_PROBES = 256
KEEP_VECTOR_LISTS = 0xFFFFFFFF
MAX_VECTOR_TRAIN_ITERS = 256
VECTOR_TRAIN_CHUNK = 256
SHARD_UNIQUE_ID_BYTES = 128

OK, ERR_INVALID, ERR_DEVICE, ERR_OOM, ERR_UNSUPPORTED, ERR_INTERNAL = 0, -1, -2, -3, -4, -5
STRATEGY_BM25, STRATEGY_WAND, STRATEGY_BMW = 0, 1, 2
METRIC_COSINE, METRIC_L2 = 0, 1
PLAN_SUM, PLAN_DISMAX, PLAN_LEAF = 0, 1, 2
MAX_SORT_PARTS = 4
SORT_SCORE = -1
ORDER_ASC, ORDER_DESC = 0, 1
MAX_AGGS = 8
MAX_AGG_RANGES = 16
MAX_AGG_CELLS = 65536
AGG_LDS_BYTES = 32768
AGG_TERMS, AGG_HISTOGRAM, AGG_RANGE, AGG_STATS = 0, 1, 2, 3
AGG_CARDINALITY, AGG_PERCENTILES, AGG_PERCENTILE_RANKS = 4, 5, 6
AGG_DATE_HISTOGRAM, AGG_FILTER = 8, 9  # (7 is not a kind)
DATE_FIXED, DATE_DAY, DATE_WEEK, DATE_MONTH, DATE_QUARTER, DATE_YEAR = 0, 1, 2, 3, 4, 5
MAX_AGG_SCRATCH_WORDS = 1 << 19
AGG_PCT_LDS_BYTES = 16384
MAX_AGG_RANKS = 1 << 24
MAX_TOP_HITS_NODES = 4
MAX_TOP_HITS = 64
MAX_TOP_HITS_CELLS = 65536
MAX_TOP_HITS_ENTRIES = 1 << 19
MAX_COMPOSITE_SOURCES = 4
MAX_COMPOSITE_SIZE = 1024
COMPOSITE_TERMS, COMPOSITE_HISTOGRAM = 0, 1
COMPOSITE_MIN_CAP = 512  # slg::kCpMinCap: entries of the smallest per-wave key set of composite_select_kernel


def composite_cap(size: int) -> int:
    """slg::cp_cap: entries of one wave's key set for a request of `size` buckets (a power of two >= 2 * (size + 1));
    the set is compacted when it holds more than 3/4 of that (slg::cp_fill_limit)"""
    cap = COMPOSITE_MIN_CAP
    while cap < 2 * (size + 1):
        cap <<= 1
    return cap


MAX_TERM_BUCKET_NODES = 4
MAX_TERM_BUCKET_SIZE = 1024
TERMS_SIGNIFICANT, TERMS_RARE = 0, 1
term_bucket_cap = composite_cap  # term_bucket_select_kernel keeps composite_select_kernel's per-wave set


RESCORE_TOTAL, RESCORE_MULTIPLY, RESCORE_SUM, RESCORE_MAX, RESCORE_MIN = 0, 1, 2, 3, 4
MAX_RESCORE_WINDOW = 1024
BOOL_MUST, BOOL_SHOULD, BOOL_MUST_NOT = 0, 1, 2
MAX_BOOL_GROUPS = 32
MAX_BOOL_TERMS = 64
MAX_BOOL_TREE_LEAVES = 32
MAX_BOOL_TREE_NODES = 32
MAX_PHRASE_TERMS = 8
MAX_PHRASE_VARIANTS = 8
MAX_PHRASE_QUERY_TERMS = 64
MAX_PHRASE_SLOP = 2147483647 - 8
MAX_FSCORE_FUNCS = 8
FSCORE_WEIGHT, FSCORE_FIELD_VALUE_FACTOR, FSCORE_DECAY = 0, 1, 2
FSCORE_MOD_NONE, FSCORE_MOD_LOG, FSCORE_MOD_LOG1P, FSCORE_MOD_LOG2P, FSCORE_MOD_SQRT, FSCORE_MOD_RECIPROCAL = 0, 1, 2, 3, 4, 5
FSCORE_DECAY_EXP, FSCORE_DECAY_GAUSS, FSCORE_DECAY_LINEAR = 0, 1, 2
FSCORE_MODE_SUM, FSCORE_MODE_MULTIPLY, FSCORE_MODE_MAX, FSCORE_MODE_MIN, FSCORE_MODE_AVG = 0, 1, 2, 3, 4
FSCORE_BOOST_MULTIPLY, FSCORE_BOOST_SUM, FSCORE_BOOST_REPLACE, FSCORE_BOOST_MAX, FSCORE_BOOST_MIN = 0, 1, 2, 3, 4
FSCORE_HAS_MAX_BOOST, FSCORE_HAS_MIN_SCORE = 1, 2
MAX_SCRIPT_INSTRS, MAX_SCRIPT_DEPTH, MAX_SCRIPT_FIELDS = 64, 8, 8
SCRIPT_PUSH_CONST, SCRIPT_PUSH_FIELD, SCRIPT_PUSH_SCORE, SCRIPT_ADD, SCRIPT_SUB, SCRIPT_MUL, SCRIPT_DIV, SCRIPT_NEG = range(8)
SCRIPT_OUTER, SCRIPT_INNER = 0, 1
SCAN_MATCH_ALL, SCAN_CONSTANT, SCAN_RANK_FEATURE = 0, 1, 2
SCAN_MOD_NONE, SCAN_MOD_LOG, SCAN_MOD_LOG1P, SCAN_MOD_SQRT, SCAN_MOD_RECIPROCAL = 0, 1, 2, 3, 4
FILTER_KEYWORD_IN, FILTER_RANGE_F64, FILTER_RANGE_I64, FILTER_ID, FILTER_AND, FILTER_OR, FILTER_NOT = 0, 1, 2, 3, 4, 5, 6
MAX_FILTER_NODES, MAX_FILTER_DEPTH, MAX_FILTER_TREES = 64, 16, 64
FILTER_NESTED = 7
MAX_NESTED_SCOPES, MAX_NESTED_DEPTH = 16, 4
MAX_COLLAPSE_ROWS = 4096
MAX_INNER_HITS = 64
EXPAND_FUZZY, EXPAND_PREFIX, EXPAND_WILDCARD = 0, 1, 2
EXPAND_REGEX = 4                                 # (3 is reserved: an unknown kind)
MAX_REGEX_STATES, MAX_REGEX_TABLE = 256, 16384   # a pattern's minimised DFA: states, states x byte classes
MAX_EXPAND_CHARS = 128
MAX_EXPANSIONS = 1024
EXPAND_WAVE, EXPAND_WORKGROUP, EXPAND_CHUNK = 64, 256, 1024  # the scan's geometry (SLG_EXPAND_*)
MAX_SUGGEST_CANDIDATES, SUGGEST_MIN_SCAN, SUGGEST_MERGE_WORKGROUP = 256, 64, 256  # slg_suggest_batch (SLG_*)
MAX_HL_TERMS, MAX_HL_PHRASES, MAX_HL_TAG, MAX_HL_FRAGMENT, MAX_HL_FRAGMENTS = 32, 8, 64, 1024, 8  # highlighting (SLG_MAX_HL_*)
HL_OK, HL_HOST, HL_NO_TEXT = 0, 1, 2


class SlgError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"searchlite_gpu error {code}: {msg}")
        self.code = code
        self.msg = msg


class SegmentDesc(C.Structure):
    _fields_ = [("n_docs", C.c_uint32), ("n_terms", C.c_uint32),
                ("term_offsets", C.c_void_p), ("doc_ids", C.c_void_p), ("tfs", C.c_void_p),
                ("term_field", C.c_void_p), ("n_fields", C.c_uint32),
                ("field_doc_len", C.c_void_p), ("field_avgdl", C.c_void_p),
                ("docs", C.c_float), ("k1", C.c_float), ("b", C.c_float),
                ("deleted", C.c_void_p),
                ("vec_dim", C.c_uint32), ("vec_metric", C.c_int32),
                ("vec_offsets", C.c_void_p), ("vec_values", C.c_void_p),
                ("vec_rows", C.c_uint32)]


class VectorFieldDesc(C.Structure):
    _fields_ = [("vec_dim", C.c_uint32), ("vec_metric", C.c_int32), ("vec_offsets", C.c_void_p),
                ("vec_values", C.c_void_p), ("vec_rows", C.c_uint32)]


class VectorListsDesc(C.Structure):
    _fields_ = [("n_lists", C.c_uint32), ("centroids", C.c_void_p)]


class VectorTrainDesc(C.Structure):
    _fields_ = [("n_lists", C.c_uint32), ("iters", C.c_uint32), ("init", C.c_void_p)]


class VectorTrainStats(C.Structure):
    _fields_ = [("iters_run", C.c_uint32), ("moved", C.c_uint32), ("empty_lists", C.c_uint32),
                ("max_len", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("scored_docs", C.c_uint64), ("candidates_examined", C.c_uint64),
                ("postings_advanced", C.c_uint64)]


class Tuning(C.Structure):
    """slg_tuning: planner knobs fixed per index (include/searchlite_gpu.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("validate", C.c_int32), ("champions", C.c_int32),
                ("allow_any_arch", C.c_int32), ("pruning", C.c_int32),
                ("uniform_max_terms", C.c_uint32), ("uniform_round_target", C.c_uint32),
                ("multi_round_target", C.c_uint32), ("probe_target", C.c_uint32),
                ("rounds_per_slice", C.c_uint32), ("max_rounds_per_slice", C.c_uint32),
                ("slices_per_subquery", C.c_uint32), ("cand_mode", C.c_int32),
                ("slice_order", C.c_int32), ("block_max", C.c_int32), ("pool_cap_mb", C.c_uint32),
                ("uniform_kernel", C.c_uint32), ("uniform_sigma_x100", C.c_uint32),
                ("inline_cuts", C.c_int32), ("updatable", C.c_int32),
                ("uniform_plans", C.c_int32), ("score_waves_per_simd", C.c_uint32)]


class ScorePlans(C.Structure):
    """slg_score_plans: flat (leaf_group NULL) or two-level score plans."""
    _fields_ = [("q_leaf", C.c_void_p), ("q_plan", C.c_void_p), ("q_tie", C.c_void_p), ("q_nleaves", C.c_void_p),
                ("q_leaf_offsets", C.c_void_p), ("leaf_group", C.c_void_p), ("q_group_offsets", C.c_void_p),
                ("group_plan", C.c_void_p), ("group_tie", C.c_void_p),
                ("q_node_offsets", C.c_void_p), ("node_kind", C.c_void_p), ("node_tie", C.c_void_p),
                ("node_parent", C.c_void_p), ("q_min_match", C.c_void_p)]


class SortSpec(C.Structure):
    """slg_sort_spec: the parts of a field sort (sort field id or SORT_SCORE, ORDER_*)."""
    _fields_ = [("n_parts", C.c_uint32), ("field", C.c_int32 * MAX_SORT_PARTS), ("order", C.c_int32 * MAX_SORT_PARTS)]


class SortCursor(C.Structure):
    """slg_sort_cursor: a query's cursor key (slg_batch_prepare_after): has_cursor, the last hit's segment and
    doc, the Missing parts, and per part an i64 value, f64 bits or (low 32 bits) a score's f32 bits."""
    _fields_ = [("has_cursor", C.c_uint32), ("segment_ord", C.c_uint32), ("doc_id", C.c_uint32),
                ("missing_mask", C.c_uint32), ("value_bits", C.c_uint64 * MAX_SORT_PARTS)]


class AggNode(C.Structure):
    """slg_agg_node: one aggregation node (AGG_* kind, agg field id, parent = -1 or an earlier bucket root)."""
    _fields_ = [("kind", C.c_int32), ("field", C.c_int32), ("parent", C.c_int32), ("has_missing", C.c_uint32),
                ("missing", C.c_double), ("missing_ord", C.c_uint32), ("has_hard_bounds", C.c_uint32),
                ("interval", C.c_double), ("offset", C.c_double), ("hard_min", C.c_double), ("hard_max", C.c_double),
                ("n_ranges", C.c_uint32), ("from_", C.c_double * MAX_AGG_RANGES), ("to", C.c_double * MAX_AGG_RANGES),
                # date_histogram: DATE_* and i64 milliseconds (has_hard_bounds, has_missing / missing as above);
                # filter: a registered filter id
                ("calendar_unit", C.c_uint32), ("filter", C.c_int32), ("date_step", C.c_int64),
                ("date_offset", C.c_int64), ("date_hard_min", C.c_int64), ("date_hard_max", C.c_int64)]


class AggSpec(C.Structure):
    """slg_agg_spec: the nodes of a batch's aggregations, roots and children together."""
    _fields_ = [("n_nodes", C.c_uint32), ("nodes", AggNode * MAX_AGGS)]


class TopHitsNode(C.Structure):
    """slg_top_hits_node: parent = -1 (the root) or a root bucket node of the aggregation spec, the rows
    [from, from + size) of the list, the node's sort (n_parts 0: `_score` desc)."""
    _fields_ = [("parent", C.c_int32), ("from_", C.c_uint32), ("size", C.c_uint32), ("sort", SortSpec)]


class TopHitsSpec(C.Structure):
    """slg_top_hits_spec: the top_hits nodes of a batch, next to its aggregation spec; max_entries 0 = the default
    capacity of a query's bucket runs."""
    _fields_ = [("n_nodes", C.c_uint32), ("max_entries", C.c_uint32), ("nodes", TopHitsNode * MAX_TOP_HITS_NODES)]


class TopHitsLayout(C.Structure):
    """slg_top_hits_layout: a node's hits are lists x size cells at hit_offset, its counts `lists` at list_offset."""
    _fields_ = [("lists", C.c_uint32), ("size", C.c_uint32), ("list_offset", C.c_uint32), ("hit_offset", C.c_uint32)]


class CompositeSource(C.Structure):
    """slg_composite_source: COMPOSITE_* kind, agg field id, the interval of a histogram source, the rank of every
    ordinal's key in byte order for a terms source (NULL: the ordinals are in key order)."""
    _fields_ = [("kind", C.c_uint32), ("field", C.c_int32), ("interval", C.c_double), ("ord_rank", C.c_void_p)]


class CompositeSpec(C.Structure):
    """slg_composite_spec: the sources in request order, the page size, the children (parent is not read)."""
    _fields_ = [("n_sources", C.c_uint32), ("size", C.c_uint32), ("sources", CompositeSource * MAX_COMPOSITE_SOURCES),
                ("n_children", C.c_uint32), ("children", AggNode * MAX_AGGS)]


class AggLayout(C.Structure):
    """slg_agg_layout: a node's table is parent_rows x rows at `offset` of the count (is_stats 0), the stats (1) or
    the value table (2)."""
    _fields_ = [("parent_rows", C.c_uint32), ("rows", C.c_uint32), ("first_id", C.c_int64),
                ("is_stats", C.c_uint32), ("offset", C.c_uint64)]


class AggStats(C.Structure):
    """slg_agg_stats: one stats cell."""
    _fields_ = [("count", C.c_uint64), ("min", C.c_double), ("max", C.c_double), ("sum", C.c_double)]


class RescoreSpec(C.Structure):
    """slg_rescore_spec: the rescore queries (CSR, flat plan arrays), their windows and score modes."""
    _fields_ = [("q_offsets", C.c_void_p), ("q_term_ids", C.c_void_p), ("q_weights", C.c_void_p),
                ("q_leaf", C.c_void_p), ("q_plan", C.c_void_p), ("q_tie", C.c_void_p), ("q_nleaves", C.c_void_p),
                ("q_min_match", C.c_void_p), ("q_window", C.c_void_p), ("q_mode", C.c_void_p)]


class BoolSpec(C.Structure):
    """slg_bool_spec: the clause tables of a bool batch (CSR clause terms with their groups, group kinds,
    minimum_should_match per query)."""
    _fields_ = [("c_offsets", C.c_void_p), ("c_term_ids", C.c_void_p), ("c_group", C.c_void_p),
                ("g_offsets", C.c_void_p), ("g_kind", C.c_void_p), ("q_min_should", C.c_void_p)]


class BoolTreeSpec(C.Structure):
    """slg_bool_tree_spec: the matcher trees of a tree batch (CSR clause terms with their term groups, filter leaves,
    and per query a post-order node table of (child, kind) edges with a min_should per node)."""
    _fields_ = [("c_offsets", C.c_void_p), ("c_term_ids", C.c_void_p), ("c_group", C.c_void_p),
                ("g_offsets", C.c_void_p), ("f_offsets", C.c_void_p), ("f_filter", C.c_void_p),
                ("n_offsets", C.c_void_p), ("n_min_should", C.c_void_p), ("e_offsets", C.c_void_p),
                ("e_child", C.c_void_p), ("e_kind", C.c_void_p)]


class PhraseSpec(C.Structure):
    """slg_phrase_spec: the phrase groups of a phrase batch (CSR: phrases per query, variants per phrase, term
    rows per variant; minimum_should_match per query over term and phrase groups)."""
    _fields_ = [("p_offsets", C.c_void_p), ("p_kind", C.c_void_p), ("p_slop", C.c_void_p), ("v_offsets", C.c_void_p),
                ("t_offsets", C.c_void_p), ("t_term_ids", C.c_void_p), ("q_min_should", C.c_void_p)]


class FscoreSpec(C.Structure):
    """slg_fscore_spec: the function_score of every query of a batch (CSR functions; score mode, boost mode,
    max_boost / min_score behind their flags, and boost per query)."""
    _fields_ = [("q_fn_offsets", C.c_void_p), ("q_score_mode", C.c_void_p), ("q_boost_mode", C.c_void_p),
                ("q_flags", C.c_void_p), ("q_max_boost", C.c_void_p), ("q_min_score", C.c_void_p),
                ("q_boost", C.c_void_p), ("f_kind", C.c_void_p), ("f_field", C.c_void_p), ("f_filter", C.c_void_p),
                ("f_weight", C.c_void_p), ("f_modifier", C.c_void_p), ("f_decay_fn", C.c_void_p),
                ("f_missing", C.c_void_p), ("f_origin", C.c_void_p), ("f_scale", C.c_void_p),
                ("f_offset", C.c_void_p), ("f_decay", C.c_void_p)]


class ScriptSpec(C.Structure):
    """slg_script_spec: the script_score program of every query of a batch (CSR instructions in reverse Polish
    order, their constants, and boost per query)."""
    _fields_ = [("p_offsets", C.c_void_p), ("i_op", C.c_void_p), ("i_arg", C.c_void_p), ("consts", C.c_void_p),
                ("n_consts", C.c_uint32), ("q_boost", C.c_void_p)]


class ScanSpec(C.Structure):
    """slg_scan_spec: the unscored root node of every query of a scan batch (match_all, constant_score,
    rank_feature): kind, the node's own filter, and the arguments of its kind, per query."""
    _fields_ = [("q_kind", C.c_void_p), ("q_filter", C.c_void_p), ("q_score", C.c_void_p), ("q_field", C.c_void_p),
                ("q_modifier", C.c_void_p), ("q_missing", C.c_void_p), ("q_boost", C.c_void_p)]


class CollapseSpec(C.Structure):
    """slg_collapse_spec: the keyword column whose ordinals are the group keys, the groups reported per query, the
    inner hits' from / size (size 0: none) and their sort (NULL: the batch's own order)."""
    _fields_ = [("field", C.c_int32), ("group_limit", C.c_uint32), ("inner_from", C.c_uint32),
                ("inner_size", C.c_uint32), ("inner_sort", C.c_void_p)]


class Request(C.Structure):
    """slg_request: the query arrays and one nullable pointer per batch kind (slg_batch_prepare_request); a kind
    is asked for when its pointer is set.  struct_size = sizeof."""
    _fields_ = [("struct_size", C.c_uint32), ("nq", C.c_uint32), ("q_offsets", C.c_void_p), ("q_term_ids", C.c_void_p),
                ("q_weights", C.c_void_p), ("plans", C.c_void_p), ("q_filter", C.c_void_p), ("k", C.c_uint32),
                ("strategy", C.c_int32), ("sort", C.c_void_p), ("q_cursor", C.c_void_p), ("bool_spec", C.c_void_p),
                ("phrase_spec", C.c_void_p), ("bool_tree_spec", C.c_void_p), ("fscore_spec", C.c_void_p),
                ("script_spec", C.c_void_p), ("script_order", C.c_int32), ("reserved", C.c_uint32),
                ("aggs", C.c_void_p), ("top_hits", C.c_void_p), ("composite", C.c_void_p),
                ("term_buckets", C.c_void_p), ("rescore", C.c_void_p), ("collapse", C.c_void_p)]


class FilterNode(C.Structure):
    """slg_filter_node: one node of a filter tree's postfix program (slg_index_add_filter_trees)."""
    _fields_ = [("kind", C.c_int32), ("field", C.c_int32), ("filter_id", C.c_int32), ("arity", C.c_uint32),
                ("lo_f", C.c_double), ("hi_f", C.c_double), ("lo_i", C.c_int64), ("hi_i", C.c_int64),
                ("ord_begin", C.c_uint32), ("n_ords_in", C.c_uint32)]


class FilterTree(C.Structure):
    """slg_filter_tree: the nodes of one tree and the ordinals its KEYWORD_IN nodes point into."""
    _fields_ = [("n_nodes", C.c_uint32), ("nodes", C.c_void_p), ("n_ords", C.c_uint32), ("ords", C.c_void_p)]


class NestedScope(C.Structure):
    """slg_nested_scope: one scope of a nested filter tree; path -1 is the doc level (the last scope)."""
    _fields_ = [("path", C.c_int32), ("node_begin", C.c_uint32), ("n_nodes", C.c_uint32)]


class NestedFilterTree(C.Structure):
    """slg_nested_filter_tree: the scopes of one tree (children before parents), their nodes and the ordinals."""
    _fields_ = [("n_scopes", C.c_uint32), ("scopes", C.c_void_p), ("n_nodes", C.c_uint32), ("nodes", C.c_void_p),
                ("n_ords", C.c_uint32), ("ords", C.c_void_p)]


class ExpandReq(C.Structure):
    """slg_expand_req: one term / prefix / wildcard pattern to expand (slg_expand_batch)."""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_int32), ("field", C.c_char_p), ("term", C.c_char_p),
                ("field_len", C.c_uint32), ("term_len", C.c_uint32), ("max_expansions", C.c_uint32),
                ("max_edits", C.c_uint32), ("prefix_length", C.c_uint32), ("min_length", C.c_uint32)]


class SuggestReq(C.Structure):
    """slg_suggest_req: one completion request (slg_suggest_batch)."""
    _fields_ = [("struct_size", C.c_uint32), ("field", C.c_char_p), ("term", C.c_char_p), ("field_len", C.c_uint32),
                ("term_len", C.c_uint32), ("size", C.c_uint32), ("has_fuzzy", C.c_uint32), ("max_edits", C.c_uint32),
                ("prefix_length", C.c_uint32), ("max_expansions", C.c_uint32), ("min_length", C.c_uint32)]


class HlSpec(C.Structure):
    """slg_hl_spec: one field spec of one query (slg_highlight_batch / slg_batch_highlight)."""
    _fields_ = [("struct_size", C.c_uint32), ("text_field", C.c_int32), ("n_terms", C.c_uint32), ("n_phrases", C.c_uint32),
                ("phrase_offsets", C.c_void_p), ("word_offsets", C.c_void_p), ("word_bytes", C.c_void_p),
                ("pre_tag", C.c_void_p), ("post_tag", C.c_void_p), ("pre_len", C.c_uint32), ("post_len", C.c_uint32),
                ("fragment_size", C.c_uint32), ("number_of_fragments", C.c_uint32)]


class HlOut(C.Structure):
    """slg_hl_out: the capacities and arrays of a highlight call, and the totals it fills."""
    _fields_ = [("struct_size", C.c_uint32), ("item_capacity", C.c_uint32), ("frag_capacity", C.c_uint32),
                ("text_capacity", C.c_uint64), ("status", C.c_void_p), ("offsets", C.c_void_p),
                ("text_offsets", C.c_void_p), ("text", C.c_void_p), ("n_items", C.c_uint32), ("n_frags", C.c_uint32),
                ("text_bytes", C.c_uint64)]


MAX_EXPLAIN_ROWS, MAX_EXPLAIN_FUNCS = 1024, 9  # SLG_MAX_EXPLAIN_*
(EXPLAIN_WEIGHT, EXPLAIN_FIELD_VALUE_FACTOR, EXPLAIN_DECAY_EXP, EXPLAIN_DECAY_GAUSS, EXPLAIN_DECAY_LINEAR,
 EXPLAIN_SCRIPT_SCORE) = range(6)


class ExplainOut(C.Structure):
    """slg_explain_out: the caller's arrays of slg_batch_explain, a stride of `rows` per query."""
    _fields_ = [("base_score", C.c_void_p), ("final_score", C.c_void_p), ("n_functions", C.c_void_p),
                ("fn_type", C.c_void_p), ("fn_field", C.c_void_p), ("fn_value", C.c_void_p),
                ("rescored", C.c_void_p), ("rescore_score", C.c_void_p), ("combined_score", C.c_void_p)]


class Ticket(C.Structure):
    """slg_ticket (slg_coalescer_submit / _wait)."""
    _fields_ = [("batch", C.c_void_p), ("row", C.c_uint32), ("k", C.c_uint32), ("kind", C.c_uint32)]


class Query(C.Structure):
    _fields_ = [("n_terms", C.c_uint32), ("term_ids", C.c_void_p), ("weights", C.c_void_p)]


_lib = None


def lib_path() -> str:
    """The product library; SLG_LIB_TAG=<tag> selects an experiment build
    libsearchlite_gpu_<tag>.so (tools/build_variant.sh, A/B timing on one box)."""
    tag = os.environ.get("SLG_LIB_TAG")
    if tag:
        return os.path.join(_build.LIBDIR, f"libsearchlite_gpu_{tag}.so")
    return _build.GPU_LIB


class CompositeSourceLayout(C.Structure):
    """slg_composite_source_layout: the part of a source in the packed key; zero_slot is the slot of -0.0."""
    _fields_ = [("shift", C.c_uint32), ("bits", C.c_uint32), ("slots", C.c_uint64), ("first_id", C.c_int64),
                ("zero_slot", C.c_int64)]


class CompositeLayout(C.Structure):
    """slg_composite_layout: the packed key, the composite's count cells and its children's tables in a query's rows."""
    _fields_ = [("n_sources", C.c_uint32), ("size", C.c_uint32), ("key_bits", C.c_uint32), ("n_children", C.c_uint32),
                ("sources", CompositeSourceLayout * MAX_COMPOSITE_SOURCES), ("count_offset", C.c_uint64),
                ("children", AggLayout * MAX_AGGS)]


class TermBucketNode(C.Structure):
    """slg_term_bucket_node: TERMS_* kind, keyword agg field id, size, min_doc_count (significant) or max_doc_count
    (rare), the background filter id of a significant node (-1: none), the rank of every ordinal's key in byte order
    (NULL: the ordinals are in key order), the children (parent is not read)."""
    _fields_ = [("kind", C.c_uint32), ("field", C.c_int32), ("size", C.c_uint32), ("doc_count_bound", C.c_uint64),
                ("background_filter", C.c_int32), ("ord_rank", C.c_void_p), ("n_children", C.c_uint32),
                ("children", AggNode * MAX_AGGS)]


class TermBucketSpec(C.Structure):
    """slg_term_bucket_spec: the significant_terms / rare_terms nodes of a request."""
    _fields_ = [("n_nodes", C.c_uint32), ("nodes", TermBucketNode * MAX_TERM_BUCKET_NODES)]


class TermBucketNodeLayout(C.Structure):
    """slg_term_bucket_node_layout: a node's rows in a query's output rows, its count cells and children's tables."""
    _fields_ = [("size", C.c_uint32), ("n_children", C.c_uint32), ("row_offset", C.c_uint64),
                ("count_offset", C.c_uint64), ("children", AggLayout * MAX_AGGS)]


class TermBucketLayout(C.Structure):
    """slg_term_bucket_layout: the nodes' layouts; rows = the output rows of one query."""
    _fields_ = [("n_nodes", C.c_uint32), ("rows", C.c_uint32), ("nodes", TermBucketNodeLayout * MAX_TERM_BUCKET_NODES)]


def load():
    """Load libsearchlite_gpu.so (built by searchlite_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
            "searchlite_amd has no CPU fallback.")
    if os.environ.get("SLG_NO_TORCH_PRELOAD", "0") == "0":
        # PyTorch-ROCm bundles its own libamdhip64/libhsa-runtime64.  Two HIP runtimes in one
        # process do not share the GPU (the second to initialise reports "no HIP GPUs"), so
        # when torch is installed load it first: libsearchlite_gpu.so then binds to the HIP
        # runtime that is already resident (same SONAME).
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(path)
    vp, u32, i32, f32 = C.c_void_p, C.c_uint32, C.c_int, C.c_float
    sigs = {
        "slg_abi_version": (u32, []),
        "slg_last_error": (C.c_char_p, []),
        "slg_last_error_code": (i32, []),
        "slg_tuning_default": (None, [vp]),
        "slg_index_create_tuned": (vp, [vp, u32, i32, vp]),
        "slg_index_get_tuning": (i32, [vp, vp]),
        "slg_device_count": (i32, []),
        "slg_index_create": (vp, [vp, u32, i32]),
        "slg_index_destroy": (None, [vp]),
        "slg_index_info": (i32, [vp, vp, vp, vp]),
        "slg_index_fetch_champions": (i32, [vp, u32, vp]),
        "slg_index_trim_pool": (i32, [vp, vp]),
        "slg_index_set_stream": (i32, [vp, vp]),
        "slg_index_update_deleted": (i32, [vp, u32, vp, f32]),
        "slg_index_add_segment": (i32, [vp, vp]),
        "slg_index_remove_segment": (i32, [vp, u32]),
        "slg_index_generation": (C.c_uint64, [vp]),
        "slg_index_device": (i32, [vp]),
        "slg_coalescer_create": (vp, [vp, u32, u32]),
        "slg_coalescer_destroy": (None, [vp]),
        "slg_coalescer_search": (i32, [vp, vp, u32, i32, vp, vp, vp, vp, vp]),
        "slg_coalescer_search_plan": (i32, [vp, vp, vp, i32, f32, u32, C.c_int32, u32, i32, vp, vp, vp, vp, vp]),
        "slg_coalescer_submit": (i32, [vp, vp, vp, i32, f32, u32, C.c_int32, u32, i32, i32, vp]),
        "slg_coalescer_poll": (i32, [vp, vp]),
        "slg_coalescer_wait": (i32, [vp, vp, vp, vp, vp, vp, vp]),
        "slg_coalescer_last_error": (C.c_char_p, []),
        "slg_coalescer_stats": (i32, [vp, vp, vp]),
        "slg_coalescer_phase_ms": (i32, [vp, vp, vp, vp, vp]),
        "slg_search_batch": (i32, [vp, vp, u32, u32, i32, vp, vp, vp, vp, vp]),
        "slg_index_add_filter": (i32, [vp, vp]),
        "slg_index_add_filter_terms": (i32, [vp, vp, u32, i32, vp]),
        "slg_index_add_filter_range_i64": (i32, [vp, vp, C.c_int64, C.c_int64]),
        "slg_index_add_filter_range_f64": (i32, [vp, vp, C.c_double, C.c_double]),
        "slg_index_remove_filter": (i32, [vp, i32]),
        "slg_search_batch_filtered": (i32, [vp, vp, u32, vp, u32, i32, vp, vp, vp, vp, vp]),
        "slg_batch_prepare": (vp, [vp, u32, vp, vp, vp, u32, i32]),
        "slg_batch_prepare_filtered": (vp, [vp, u32, vp, vp, vp, vp, u32, i32]),
        "slg_batch_prepare_plan": (vp, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, i32]),
        "slg_batch_prepare_plans": (vp, [vp, u32, vp, vp, vp, vp, vp, u32, i32]),
        "slg_index_add_sort_field_i64": (i32, [vp, vp, vp]),
        "slg_index_add_sort_field_f64": (i32, [vp, vp, vp]),
        "slg_index_remove_sort_field": (i32, [vp, i32]),
        "slg_batch_prepare_sorted": (vp, [vp, u32, vp, vp, vp, vp, vp, vp, u32, i32]),
        "slg_batch_matched_counts": (i32, [vp, vp]),
        "slg_search_batch_sorted": (i32, [vp, vp, u32, vp, vp, vp, u32, i32, vp, vp, vp, vp, vp]),
        "slg_batch_prepare_after": (vp, [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, i32]),
        "slg_batch_cursor_seen": (i32, [vp, vp]),
        "slg_search_batch_after": (i32, [vp, vp, u32, vp, vp, vp, vp, u32, i32, vp, vp, vp, vp, vp, vp]),
        "slg_index_add_agg_field_f64": (i32, [vp, vp, vp]),
        "slg_index_add_agg_field_i64": (i32, [vp, vp, vp]),
        "slg_index_add_agg_field_ord": (i32, [vp, vp, vp, u32]),
        "slg_index_remove_agg_field": (i32, [vp, i32]),
        "slg_index_rank_agg_field": (C.c_int64, [vp, i32]),
        "slg_batch_prepare_aggs": (vp, [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, i32]),
        "slg_batch_agg_layout": (i32, [vp, vp]),
        "slg_batch_fetch_aggs": (i32, [vp, vp, vp]),
        "slg_batch_fetch_agg_values": (i32, [vp, vp]),
        "slg_search_batch_agg_values": (i32, [vp, vp, u32, vp, vp, vp, vp, u32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "slg_search_batch_aggs": (i32, [vp, vp, u32, vp, vp, vp, vp, u32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "slg_batch_prepare_top_hits": (vp, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, i32]),
        "slg_batch_top_hits_layout": (i32, [vp, vp]),
        "slg_batch_fetch_top_hits": (i32, [vp] * 6),
        "slg_search_batch_top_hits": (i32, [vp, vp, u32, vp, vp, vp, vp, vp, u32, i32] + [vp] * 13),
        "slg_batch_prepare_composite": (vp, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, i32]),
        "slg_batch_composite_layout": (i32, [vp, vp]),
        "slg_batch_set_composite_after": (i32, [vp, vp]),
        "slg_batch_fetch_composite": (i32, [vp] * 4),
        "slg_search_batch_composite": (i32, [vp, vp, u32, vp, vp, vp, vp, vp, u32, i32] + [vp] * 10),
        "slg_batch_prepare_term_buckets": (vp, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, i32]),
        "slg_batch_term_buckets_layout": (i32, [vp, vp]),
        "slg_batch_fetch_term_buckets": (i32, [vp] * 8),
        "slg_search_batch_term_buckets": (i32, [vp, vp, u32, vp, vp, vp, vp, vp, u32, i32] + [vp] * 14),
        "slg_batch_run": (i32, [vp]),
        "slg_batch_set_stream": (i32, [vp, vp]),
        "slg_batch_sync": (i32, [vp]),
        "slg_batch_fetch": (i32, [vp, vp, vp, vp, vp, vp]),
        "slg_batch_device_results": (i32, [vp, vp, vp, vp, vp]),
        "slg_batch_device_result_block": (i32, [vp, vp, vp]),
        "slg_batch_info": (i32, [vp, vp, vp, vp]),
        "slg_batch_skip_counts": (i32, [vp, vp, vp]),
        "slg_batch_destroy": (None, [vp]),
        "slg_merge_shards_device": (i32, [vp, u32, u32, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp]),
        "slg_shard_unique_id": (i32, [vp, C.c_size_t]),
        "slg_shard_group_create": (vp, [vp, i32, i32, vp, u32]),
        "slg_shard_group_destroy": (None, [vp]),
        "slg_batch_run_sharded": (i32, [vp, vp, vp, vp, vp, vp]),
        "slg_batch_sharded_device_results": (i32, [vp, vp, vp, vp, vp]),
        "slg_batch_run_sharded_seq": (i32, [vp, vp, C.c_uint64, vp, vp, vp, vp]),
        "slg_shard_group_stats": (i32, [vp, vp, vp, vp, vp]),
        "slg_shard_group_skip_seq": (i32, [vp, C.c_uint64]),
        "slg_batch_fetch_sharded": (i32, [vp, vp, vp, vp, vp]),
        "slg_profile_enable": (i32, [vp, i32]),
        "slg_profile_read": (i32, [vp, vp, vp]),
        "slg_rerank_batch": (i32, [vp, u32, vp, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp]),
        "slg_rerank_batch_device": (i32, [vp, u32, vp, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp,
                                          vp, vp]),
        "slg_rerank_multi_batch": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp,
                                         vp, vp]),
        "slg_rerank_multi_batch_device": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, u32, u32, vp,
                                                vp, vp, vp, vp]),
        "slg_index_add_vector_field": (i32, [vp, vp, u32]),
        "slg_batch_rerank_device": (i32, [vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp]),
        "slg_rerank_fields_batch": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp,
                                          vp, vp]),
        "slg_rerank_fields_batch_device": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, vp,
                                                 vp, vp, vp, vp]),
        "slg_vector_search_batch": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp]),
        "slg_vector_search_batch_device": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp, vp,
                                                 vp, vp]),
        "slg_index_quantize_vector_field": (i32, [vp, u32]),
        "slg_index_fetch_vector_copy": (i32, [vp, u32, u32, vp, vp, u32]),
        "slg_vector_search_batch_approx": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp,
                                                 vp, vp]),
        "slg_vector_search_batch_approx_device": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp,
                                                        vp, vp, vp]),
        "slg_index_cluster_vector_field": (i32, [vp, u32, vp, u32]),
        "slg_index_fetch_vector_lists": (i32, [vp, u32, u32, vp, vp, vp, u32, u32]),
        "slg_index_train_vector_field": (i32, [vp, u32, vp, u32, vp]),
        "slg_vector_search_batch_ivf": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp,
                                              vp, vp]),
        "slg_vector_search_batch_ivf_device": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp,
                                                     vp, vp, vp]),
        "slg_batch_prepare_hybrid": (vp, [vp, u32, vp, vp, vp, vp, vp, u32, i32]),
        "slg_batch_hybrid_device": (i32, [vp, u32, vp, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp]),
        "slg_search_batch_hybrid": (i32, [vp, u32, vp, vp, vp, vp, vp, u32, i32, u32, vp, vp, vp, vp, u32, u32,
                                          vp, vp, vp, vp, vp, vp]),
        "slg_batch_prepare_rescore": (vp, [vp, u32, vp, vp, vp, vp, vp, vp, u32, i32]),
        "slg_batch_fetch_rescore": (i32, [vp, vp, vp, vp]),
        "slg_search_batch_rescore": (i32, [vp, u32, vp, vp, vp, vp, vp, vp, u32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "slg_batch_prepare_bool": (vp, [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, i32]),
        "slg_search_batch_bool": (i32, [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, i32, vp, vp, vp, vp, vp, vp]),
        "slg_batch_prepare_bool_tree": (vp, [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, i32]),
        "slg_search_batch_bool_tree": (i32, [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, i32, vp, vp, vp, vp, vp, vp]),
        "slg_index_set_positions": (i32, [vp, u32, vp, vp]),
        "slg_batch_prepare_phrase": (vp, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, i32]),
        "slg_search_batch_phrase": (i32, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, i32, vp, vp, vp, vp, vp, vp]),
        "slg_batch_prepare_fscore": (vp, [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, i32]),
        "slg_batch_fscore_info": (i32, [vp, vp, vp]),
        "slg_batch_prepare_script": (vp, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, i32, u32, i32]),
        "slg_batch_script_info": (i32, [vp, vp, vp]),
        "slg_search_batch_script": (i32, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, i32, u32, i32, vp, vp, vp, vp, vp, vp]),
        "slg_index_add_filter_trees": (i32, [vp, vp, u32, vp]),
        "slg_index_fetch_filter": (i32, [vp, i32, u32, vp]),
        "slg_index_add_nested_path": (i32, [vp, i32, vp, vp, vp]),
        "slg_index_remove_nested_path": (i32, [vp, i32]),
        "slg_index_add_nested_field_f64": (i32, [vp, i32, vp, vp, vp]),
        "slg_index_add_nested_field_i64": (i32, [vp, i32, vp, vp, vp]),
        "slg_index_add_nested_field_ord": (i32, [vp, i32, vp, vp, vp, u32]),
        "slg_index_remove_nested_field": (i32, [vp, i32]),
        "slg_index_add_nested_filter_trees": (i32, [vp, vp, u32, vp]),
        "slg_search_batch_fscore": (i32, [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, i32, vp, vp, vp, vp, vp, vp]),
        "slg_batch_prepare_scan": (vp, [vp, u32, vp, vp, vp, vp, u32]),
        "slg_batch_scan_info": (i32, [vp, vp, vp, vp]),
        "slg_search_batch_scan": (i32, [vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "slg_batch_prepare_collapse": (vp, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, i32]),
        "slg_batch_fetch_collapse": (i32, [vp] * 15),
        "slg_search_batch_collapse": (i32, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, i32] + [vp] * 18),
        "slg_batch_prepare_request": (vp, [vp, vp]),
        "slg_index_set_terms": (i32, [vp, u32, vp, vp]),
        "slg_expand_batch": (i32, [vp, vp, u32, vp, u32, vp, vp]),
        "slg_expand_phase_ms": (i32, [vp, vp, vp]),
        "slg_suggest_batch": (i32, [vp, vp, u32, vp, u32, vp, vp, vp, u32, vp]),
        "slg_suggest_phase_ms": (i32, [vp, vp, vp]),
        "slg_index_add_text_field": (i32, [vp, vp, vp]),
        "slg_index_remove_text_field": (i32, [vp, i32]),
        "slg_highlight_batch": (i32, [vp, u32, vp, vp, vp, vp, vp, vp]),
        "slg_batch_highlight": (i32, [vp, vp, vp, vp]),
        "slg_highlight_phase_ms": (i32, [vp, vp, vp]),
        "slg_batch_explain": (i32, [vp, u32, vp]),
    }
    for name, (res, args) in sigs.items():
        if os.environ.get("SLG_LIB_TAG") and not hasattr(L, name):
            continue  # an experiment build of an older revision (tools/build_variant.sh): A/B timing only
        fn = getattr(L, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def last_error() -> str:
    return load().slg_last_error().decode("utf-8", "replace")


def last_error_code() -> int:
    return int(load().slg_last_error_code())


def default_tuning() -> Tuning:
    """Defaults + SLG_* environment overrides (slg_tuning_default)."""
    t = Tuning()
    load().slg_tuning_default(C.addressof(t))
    return t


def check(rc: int) -> None:
    if rc != OK:
        raise SlgError(rc, last_error())
