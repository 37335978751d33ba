//! searchlite-core/src/gpu/ffi.rs — raw bindings of include/searchlite_gpu.h (libsearchlite_gpu.so).
//!
//! UNVERIFIED SOURCE: written against searchlite-core at the surveyed snapshot; the build image of
//! this repository has no cargo/rustc, so this file has never been compiled.  It is kept in sync
//! with the header by tests/test_abi.py (every declared function is bound here).
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_float, c_int, c_void};

#[repr(C)] pub struct slg_index { _p: [u8; 0] }
#[repr(C)] pub struct slg_batch { _p: [u8; 0] }
#[repr(C)] pub struct slg_shard_group { _p: [u8; 0] }
#[repr(C)] pub struct slg_coalescer { _p: [u8; 0] }
/// slg_coalescer_submit / _wait: one request in flight (good for one wait).
#[repr(C)] #[derive(Clone, Copy)] pub struct slg_ticket { pub batch: *mut c_void, pub row: u32, pub k: u32, pub kind: u32 }

#[repr(C)]
pub struct slg_segment_desc {
    pub n_docs: u32, pub n_terms: u32,
    pub term_offsets: *const u64, pub doc_ids: *const u32, pub tfs: *const u32,
    pub term_field: *const u16,
    pub n_fields: u32, pub field_doc_len: *const *const c_float, pub field_avgdl: *const c_float,
    pub docs: c_float, pub k1: c_float, pub b: c_float,
    pub deleted: *const u8,
    pub vec_dim: u32, pub vec_metric: i32,
    pub vec_offsets: *const u32, pub vec_values: *const c_float, pub vec_rows: u32,
}
#[repr(C)] #[derive(Clone, Copy)]
pub struct slg_tuning {
    pub struct_size: u32, pub validate: i32, pub champions: i32, pub allow_any_arch: i32, pub pruning: i32,
    pub uniform_max_terms: u32, pub uniform_round_target: u32, pub multi_round_target: u32,
    pub probe_target: u32, pub rounds_per_slice: u32, pub max_rounds_per_slice: u32,
    pub slices_per_subquery: u32, pub cand_mode: i32, pub slice_order: i32, pub block_max: i32,
    pub pool_cap_mb: u32, pub uniform_kernel: u32, pub uniform_sigma_x100: u32, pub inline_cuts: i32,
    pub updatable: i32, pub uniform_plans: i32, pub score_waves_per_simd: u32,
}
#[repr(C)] pub struct slg_vector_field_desc {
    pub vec_dim: u32, pub vec_metric: i32, pub vec_offsets: *const u32, pub vec_values: *const c_float, pub vec_rows: u32,
}
pub const SLG_MAX_VECTOR_LISTS: u32 = 65536;
pub const SLG_MAX_VECTOR_PROBES: u32 = 256;
pub const SLG_KEEP_VECTOR_LISTS: u32 = 0xFFFF_FFFF;
#[repr(C)] pub struct slg_vector_lists_desc { pub n_lists: u32, pub centroids: *const c_float }
pub const SLG_MAX_VECTOR_TRAIN_ITERS: u32 = 256;
pub const SLG_VECTOR_TRAIN_CHUNK: u32 = 256;
#[repr(C)] pub struct slg_vector_train_desc { pub n_lists: u32, pub iters: u32, pub init: *const c_float }
#[repr(C)] pub struct slg_vector_train_stats { pub iters_run: u32, pub moved: u32, pub empty_lists: u32, pub max_len: u32 }
#[repr(C)] pub struct slg_score_plans {
    pub q_leaf: *const u32, pub q_plan: *const i32, pub q_tie: *const c_float, pub q_nleaves: *const u32,
    pub q_leaf_offsets: *const u32, pub leaf_group: *const u32, pub q_group_offsets: *const u32,
    pub group_plan: *const i32, pub group_tie: *const c_float,
    // trees of any shape: per query a node array in pre-order (SLG_PLAN_SUM | _DISMAX | _LEAF)
    pub q_node_offsets: *const u32, pub node_kind: *const i32, pub node_tie: *const c_float, pub node_parent: *const u32,
    pub q_min_match: *const u32,
}
// field sorts (query/sort.rs:159-216): parts = sort field id or SLG_SORT_SCORE, order SLG_ORDER_*
#[repr(C)] pub struct slg_sort_spec {
    pub n_parts: u32, pub field: [i32; SLG_MAX_SORT_PARTS], pub order: [i32; SLG_MAX_SORT_PARTS],
}
// a query's cursor key (slg_batch_prepare_after): the CursorState key's part values (i64 two's complement, f64
// bits, or f32 bits of a score), Missing parts as bits, then segment_ord and doc_id
#[repr(C)] #[derive(Clone, Copy, Default)] pub struct slg_sort_cursor {
    pub has_cursor: u32, pub segment_ord: u32, pub doc_id: u32, pub missing_mask: u32,
    pub value_bits: [u64; SLG_MAX_SORT_PARTS],
}
// aggregations (query/aggs/mod.rs): the nodes of a batch's spec, the layout of a node's dense table, a stats cell
pub const SLG_MAX_AGGS: usize = 8;
pub const SLG_MAX_AGG_RANGES: usize = 16;
pub const SLG_MAX_AGG_CELLS: u32 = 65536;
pub const SLG_AGG_TERMS: i32 = 0;
pub const SLG_AGG_HISTOGRAM: i32 = 1;
pub const SLG_AGG_RANGE: i32 = 2;
pub const SLG_AGG_STATS: i32 = 3;
pub const SLG_AGG_CARDINALITY: i32 = 4;
pub const SLG_AGG_PERCENTILES: i32 = 5;
pub const SLG_AGG_PERCENTILE_RANKS: i32 = 6;
pub const SLG_AGG_DATE_HISTOGRAM: i32 = 8; // (7 is not a kind)
pub const SLG_AGG_FILTER: i32 = 9;
pub const SLG_DATE_FIXED: u32 = 0;
pub const SLG_DATE_DAY: u32 = 1;
pub const SLG_DATE_WEEK: u32 = 2;
pub const SLG_DATE_MONTH: u32 = 3;
pub const SLG_DATE_QUARTER: u32 = 4;
pub const SLG_DATE_YEAR: u32 = 5;
pub const SLG_MAX_AGG_SCRATCH_WORDS: u32 = 1 << 19;
pub const SLG_MAX_AGG_RANKS: u32 = 1 << 24;
#[repr(C)] #[derive(Clone, Copy)] pub struct slg_agg_node {
    pub kind: i32, pub field: i32, pub parent: i32, pub has_missing: u32, pub missing: f64, pub missing_ord: u32,
    pub has_hard_bounds: u32, pub interval: f64, pub offset: f64, pub hard_min: f64, pub hard_max: f64,
    pub n_ranges: u32, pub from: [f64; SLG_MAX_AGG_RANGES], pub to: [f64; SLG_MAX_AGG_RANGES],
    // date_histogram: SLG_DATE_* and i64 milliseconds; filter: a registered filter id
    pub calendar_unit: u32, pub filter: i32,
    pub date_step: i64, pub date_offset: i64, pub date_hard_min: i64, pub date_hard_max: i64,
}
#[repr(C)] #[derive(Clone, Copy)] pub struct slg_agg_spec { pub n_nodes: u32, pub nodes: [slg_agg_node; SLG_MAX_AGGS] }
#[repr(C)] #[derive(Clone, Copy, Default)] pub struct slg_agg_layout {
    pub parent_rows: u32, pub rows: u32, pub first_id: i64, pub is_stats: u32, pub offset: u64,
}
#[repr(C)] #[derive(Clone, Copy, Default)] pub struct slg_agg_stats { pub count: u64, pub min: f64, pub max: f64, pub sum: f64 }
// top_hits (TopHitsAggregation): the nodes travel beside the aggregation spec; a node's lists are lists x size hit
// cells (segment, doc, score) and `lists` counts
pub const SLG_MAX_TOP_HITS_NODES: usize = 4;
pub const SLG_MAX_TOP_HITS: u32 = 64;
pub const SLG_MAX_TOP_HITS_CELLS: u32 = 65536;
pub const SLG_MAX_TOP_HITS_ENTRIES: u32 = 1 << 19;
#[repr(C)] pub struct slg_top_hits_node { pub parent: i32, pub from: u32, pub size: u32, pub sort: slg_sort_spec }
#[repr(C)] pub struct slg_top_hits_spec {
    pub n_nodes: u32, pub max_entries: u32, pub nodes: [slg_top_hits_node; SLG_MAX_TOP_HITS_NODES],
}
#[repr(C)] #[derive(Clone, Copy, Default)] pub struct slg_top_hits_layout {
    pub lists: u32, pub size: u32, pub list_offset: u32, pub hit_offset: u32,
}
// composite (CompositeAggregation): the spec travels beside the aggregation spec; a tuple is one packed u64 key (source
// 0 in the most significant bits, a slot per source); the composite's `size` count cells and its children's tables lie
// behind the spec's cells in the rows of slg_batch_fetch_aggs
pub const SLG_MAX_COMPOSITE_SOURCES: usize = 4;
pub const SLG_MAX_COMPOSITE_SIZE: u32 = 1024;
pub const SLG_COMPOSITE_TERMS: u32 = 0;
pub const SLG_COMPOSITE_HISTOGRAM: u32 = 1;
#[repr(C)] pub struct slg_composite_source { pub kind: u32, pub field: i32, pub interval: f64, pub ord_rank: *const u32 }
#[repr(C)] pub struct slg_composite_spec {
    pub n_sources: u32, pub size: u32, pub sources: [slg_composite_source; SLG_MAX_COMPOSITE_SOURCES],
    pub n_children: u32, pub children: [slg_agg_node; SLG_MAX_AGGS],
}
#[repr(C)] #[derive(Clone, Copy, Default)] pub struct slg_composite_source_layout {
    pub shift: u32, pub bits: u32, pub slots: u64, pub first_id: i64, pub zero_slot: i64,
}
#[repr(C)] pub struct slg_composite_layout {
    pub n_sources: u32, pub size: u32, pub key_bits: u32, pub n_children: u32,
    pub sources: [slg_composite_source_layout; SLG_MAX_COMPOSITE_SOURCES], pub count_offset: u64,
    pub children: [slg_agg_layout; SLG_MAX_AGGS],
}
// significant_terms / rare_terms: the spec travels beside the aggregation spec; at most `size` rows per node come back
// in the response's final order; a node with children has `size` count cells and its children's tables behind the
// spec's cells in the rows of slg_batch_fetch_aggs
pub const SLG_MAX_TERM_BUCKET_NODES: usize = 4;
pub const SLG_MAX_TERM_BUCKET_SIZE: u32 = 1024;
pub const SLG_TERMS_SIGNIFICANT: u32 = 0;
pub const SLG_TERMS_RARE: u32 = 1;
#[repr(C)] pub struct slg_term_bucket_node {
    pub kind: u32, pub field: i32, pub size: u32, pub doc_count_bound: u64, pub background_filter: i32,
    pub ord_rank: *const u32, pub n_children: u32, pub children: [slg_agg_node; SLG_MAX_AGGS],
}
#[repr(C)] pub struct slg_term_bucket_spec {
    pub n_nodes: u32, pub nodes: [slg_term_bucket_node; SLG_MAX_TERM_BUCKET_NODES],
}
#[repr(C)] pub struct slg_term_bucket_node_layout {
    pub size: u32, pub n_children: u32, pub row_offset: u64, pub count_offset: u64,
    pub children: [slg_agg_layout; SLG_MAX_AGGS],
}
#[repr(C)] pub struct slg_term_bucket_layout {
    pub n_nodes: u32, pub rows: u32, pub nodes: [slg_term_bucket_node_layout; SLG_MAX_TERM_BUCKET_NODES],
}
#[repr(C)] pub struct slg_bool_spec {
    pub c_offsets: *const u32, pub c_term_ids: *const u32, pub c_group: *const u32, pub g_offsets: *const u32,
    pub g_kind: *const i32, pub q_min_should: *const u32,
}
#[repr(C)] pub struct slg_bool_tree_spec {
    pub c_offsets: *const u32, pub c_term_ids: *const u32, pub c_group: *const u32, pub g_offsets: *const u32,
    pub f_offsets: *const u32, pub f_filter: *const i32, pub n_offsets: *const u32, pub n_min_should: *const u32,
    pub e_offsets: *const u32, pub e_child: *const u32, pub e_kind: *const i32,
}
#[repr(C)] pub struct slg_fscore_spec {
    pub q_fn_offsets: *const u32, pub q_score_mode: *const i32, pub q_boost_mode: *const i32, pub q_flags: *const u32,
    pub q_max_boost: *const c_float, pub q_min_score: *const c_float, pub q_boost: *const c_float,
    pub f_kind: *const i32, pub f_field: *const i32, pub f_filter: *const i32, pub f_weight: *const c_float,
    pub f_modifier: *const i32, pub f_decay_fn: *const i32, pub f_missing: *const f64, pub f_origin: *const f64,
    pub f_scale: *const f64, pub f_offset: *const f64, pub f_decay: *const f64,
}
#[repr(C)] pub struct slg_script_spec {
    pub p_offsets: *const u32, pub i_op: *const i32, pub i_arg: *const i32, pub consts: *const f64,
    pub n_consts: u32, pub q_boost: *const c_float,
}
// scan batches: match_all, constant_score and rank_feature at the root (requests without a scored term)
pub const SLG_SCAN_MATCH_ALL: i32 = 0;
pub const SLG_SCAN_CONSTANT: i32 = 1;
pub const SLG_SCAN_RANK_FEATURE: i32 = 2;
pub const SLG_SCAN_MOD_NONE: i32 = 0;
pub const SLG_SCAN_MOD_LOG: i32 = 1;
pub const SLG_SCAN_MOD_LOG1P: i32 = 2;
pub const SLG_SCAN_MOD_SQRT: i32 = 3;
pub const SLG_SCAN_MOD_RECIPROCAL: i32 = 4;
#[repr(C)] pub struct slg_scan_spec {
    pub q_kind: *const i32, pub q_filter: *const i32, pub q_score: *const c_float, pub q_field: *const i32,
    pub q_modifier: *const i32, pub q_missing: *const c_float, pub q_boost: *const c_float,
}
#[repr(C)] pub struct slg_filter_node {
    pub kind: i32, pub field: i32, pub filter_id: i32, pub arity: u32, pub lo_f: f64, pub hi_f: f64,
    pub lo_i: i64, pub hi_i: i64, pub ord_begin: u32, pub n_ords_in: u32,
}
#[repr(C)] pub struct slg_filter_tree {
    pub n_nodes: u32, pub nodes: *const slg_filter_node, pub n_ords: u32, pub ords: *const u32,
}
#[repr(C)] pub struct slg_nested_scope {
    pub path: i32, pub node_begin: u32, pub n_nodes: u32,
}
#[repr(C)] pub struct slg_nested_filter_tree {
    pub n_scopes: u32, pub scopes: *const slg_nested_scope, pub n_nodes: u32, pub nodes: *const slg_filter_node,
    pub n_ords: u32, pub ords: *const u32,
}
#[repr(C)] pub struct slg_phrase_spec {
    pub p_offsets: *const u32, pub p_kind: *const i32, pub p_slop: *const u32, pub v_offsets: *const u32,
    pub t_offsets: *const u32, pub t_term_ids: *const u32, pub q_min_should: *const u32,
}
#[repr(C)] pub struct slg_rescore_spec {
    pub q_offsets: *const u32, pub q_term_ids: *const u32, pub q_weights: *const c_float, pub q_leaf: *const u32,
    pub q_plan: *const i32, pub q_tie: *const c_float, pub q_nleaves: *const u32, pub q_min_match: *const u32,
    pub q_window: *const u32, pub q_mode: *const i32,
}
// field collapsing (SearchRequest::collapse): the keyword column whose global ordinals are the group keys, the
// groups reported per query, the inner hits' from / size (0: none) and sort (null: the batch's own order)
#[repr(C)] pub struct slg_collapse_spec {
    pub field: i32, pub group_limit: u32, pub inner_from: u32, pub inner_size: u32,
    pub inner_sort: *const slg_sort_spec,
}
// a compound request (slg_batch_prepare_request): the query arrays and one nullable pointer per batch kind; a
// kind is asked for when its pointer is non-null; struct_size = size_of::<slg_request>()
#[repr(C)] pub struct slg_request {
    pub struct_size: u32, pub nq: u32, pub q_offsets: *const u32, pub q_term_ids: *const u32,
    pub q_weights: *const c_float, pub plans: *const slg_score_plans, pub q_filter: *const i32, pub k: u32,
    pub strategy: i32, pub sort: *const slg_sort_spec, pub q_cursor: *const slg_sort_cursor,
    pub bool_spec: *const slg_bool_spec, pub phrase_spec: *const slg_phrase_spec,
    pub bool_tree_spec: *const slg_bool_tree_spec, pub fscore_spec: *const slg_fscore_spec,
    pub script_spec: *const slg_script_spec, pub script_order: i32, pub reserved: u32,
    pub aggs: *const slg_agg_spec, pub top_hits: *const slg_top_hits_spec, pub composite: *const slg_composite_spec,
    pub term_buckets: *const slg_term_bucket_spec, pub rescore: *const slg_rescore_spec,
    pub collapse: *const slg_collapse_spec,
}
// term expansion (SearchRequest::fuzzy, QueryNode::Prefix / ::Wildcard): one source term, prefix or pattern;
// field and term are UTF-8 with byte lengths, max_edits / prefix_length / min_length are FuzzyOptions
#[repr(C)] pub struct slg_expand_req {
    pub struct_size: u32, pub kind: i32, pub field: *const c_char, pub term: *const c_char,
    pub field_len: u32, pub term_len: u32, pub max_expansions: u32,
    pub max_edits: u32, pub prefix_length: u32, pub min_length: u32,
}
#[repr(C)] pub struct slg_hl_spec {
    pub struct_size: u32, pub text_field: i32, pub n_terms: u32, pub n_phrases: u32,
    pub phrase_offsets: *const u32, pub word_offsets: *const u32, pub word_bytes: *const c_char,
    pub pre_tag: *const c_char, pub post_tag: *const c_char, pub pre_len: u32, pub post_len: u32,
    pub fragment_size: u32, pub number_of_fragments: u32,
}
#[repr(C)] pub struct slg_hl_out {
    pub struct_size: u32, pub item_capacity: u32, pub frag_capacity: u32, pub text_capacity: u64,
    pub status: *mut u8, pub offsets: *mut u32, pub text_offsets: *mut u32, pub text: *mut c_char,
    pub n_items: u32, pub n_frags: u32, pub text_bytes: u64,
}
// slg_batch_explain (SearchRequest.explain): caller-owned arrays with a stride of `rows` per query; the last three
// are read only for a rescore batch
#[repr(C)] pub struct slg_explain_out {
    pub base_score: *mut c_float, pub final_score: *mut c_float, pub n_functions: *mut u32,
    pub fn_type: *mut u32, pub fn_field: *mut i32, pub fn_value: *mut c_float,
    pub rescored: *mut u32, pub rescore_score: *mut c_float, pub combined_score: *mut c_float,
}
pub const SLG_MAX_EXPLAIN_ROWS: u32 = 1024;
pub const SLG_MAX_EXPLAIN_FUNCS: u32 = 9;
pub const SLG_EXPLAIN_WEIGHT: u32 = 0;
pub const SLG_EXPLAIN_FIELD_VALUE_FACTOR: u32 = 1;
pub const SLG_EXPLAIN_DECAY_EXP: u32 = 2;
pub const SLG_EXPLAIN_DECAY_GAUSS: u32 = 3;
pub const SLG_EXPLAIN_DECAY_LINEAR: u32 = 4;
pub const SLG_EXPLAIN_SCRIPT_SCORE: u32 = 5;
pub const SLG_HL_OK: u8 = 0;
pub const SLG_HL_HOST: u8 = 1;
pub const SLG_HL_NO_TEXT: u8 = 2;
#[repr(C)] pub struct slg_suggest_req {
    pub struct_size: u32, pub field: *const c_char, pub term: *const c_char, pub field_len: u32, pub term_len: u32,
    pub size: u32, pub has_fuzzy: u32, pub max_edits: u32, pub prefix_length: u32, pub max_expansions: u32,
    pub min_length: u32,
}
pub const SLG_MAX_SUGGEST_CANDIDATES: u32 = 256;
pub const SLG_EXPAND_FUZZY: i32 = 0;
pub const SLG_EXPAND_PREFIX: i32 = 1;
pub const SLG_EXPAND_WILDCARD: i32 = 2;
pub const SLG_EXPAND_REGEX: i32 = 4; // (3 is reserved: an unknown kind)
pub const SLG_MAX_REGEX_STATES: u32 = 256;
pub const SLG_MAX_REGEX_TABLE: u32 = 16384;
#[repr(C)] pub struct slg_stats { pub scored_docs: u64, pub candidates_examined: u64, pub postings_advanced: u64 }
#[repr(C)] pub struct slg_query { pub n_terms: u32, pub term_ids: *const u32, pub weights: *const c_float }

#[link(name = "searchlite_gpu")]
extern "C" {
    pub fn slg_abi_version() -> u32;
    pub fn slg_last_error() -> *const c_char;
    pub fn slg_last_error_code() -> c_int;
    pub fn slg_tuning_default(out: *mut slg_tuning);
    pub fn slg_index_create_tuned(segs: *const slg_segment_desc, n_segs: u32, device: c_int,
        tuning_or_null: *const slg_tuning) -> *mut slg_index;
    pub fn slg_index_get_tuning(index: *const slg_index, out: *mut slg_tuning) -> c_int;
    pub fn slg_device_count() -> c_int;
    pub fn slg_index_create(segs: *const slg_segment_desc, n_segs: u32, device: c_int) -> *mut slg_index;
    pub fn slg_index_destroy(index: *mut slg_index);
    pub fn slg_index_info(index: *const slg_index, n_segs: *mut u32, n_postings: *mut u64, device_bytes: *mut u64) -> c_int;
    // index updates: the staged index follows the manifest (api/writer.rs:106-240)
    pub fn slg_index_update_deleted(index: *mut slg_index, seg: u32, deleted: *const u8, live_docs: c_float) -> c_int;
    pub fn slg_index_add_segment(index: *mut slg_index, seg: *const slg_segment_desc) -> c_int;
    pub fn slg_index_remove_segment(index: *mut slg_index, seg: u32) -> c_int;
    pub fn slg_index_generation(index: *const slg_index) -> u64;
    pub fn slg_index_device(index: *const slg_index) -> c_int;
    // request coalescer: concurrent single-query callers -> batches (searchlite-http/src/lib.rs:628-652)
    pub fn slg_coalescer_create(index: *mut slg_index, max_batch: u32, max_wait_us: u32) -> *mut slg_coalescer;
    pub fn slg_coalescer_destroy(coalescer: *mut slg_coalescer);
    pub fn slg_coalescer_search(coalescer: *mut slg_coalescer, query: *const slg_query, k: u32, strategy: c_int,
        out_doc: *mut u32, out_seg: *mut u32, out_score: *mut c_float, out_count: *mut u32,
        stats_or_null: *mut slg_stats) -> c_int;
    pub fn slg_coalescer_search_plan(coalescer: *mut slg_coalescer, query: *const slg_query, leaf: *const u32,
        plan: c_int, tie: c_float, n_leaves: u32, filter_id: i32, k: u32, strategy: c_int, out_doc: *mut u32,
        out_seg: *mut u32, out_score: *mut c_float, out_count: *mut u32, stats_or_null: *mut slg_stats) -> c_int;
    pub fn slg_coalescer_submit(coalescer: *mut slg_coalescer, query: *const slg_query, leaf: *const u32, plan: c_int,
                                tie: f32, n_leaves: u32, filter_id: i32, k: u32, strategy: c_int, want_stats: c_int,
                                ticket: *mut slg_ticket) -> c_int;
    pub fn slg_coalescer_poll(coalescer: *const slg_coalescer, ticket: *const slg_ticket) -> c_int;
    pub fn slg_coalescer_wait(coalescer: *mut slg_coalescer, ticket: *mut slg_ticket, out_doc: *mut u32,
                              out_seg: *mut u32, out_score: *mut f32, out_count: *mut u32,
                              stats_or_null: *mut slg_stats) -> c_int;
    pub fn slg_coalescer_last_error() -> *const c_char;
    pub fn slg_coalescer_phase_ms(coalescer: *const slg_coalescer, collect: *mut f64, prepare: *mut f64, run: *mut f64,
        fetch: *mut f64) -> c_int;
    pub fn slg_coalescer_stats(coalescer: *const slg_coalescer, n_batches: *mut u64, n_queries: *mut u64) -> c_int;
    // index sharding over RCCL (api/reader.rs:2670-2778 across GPUs)
    pub fn slg_shard_unique_id(out: *mut c_void, out_bytes: usize) -> c_int;
    pub fn slg_shard_group_create(index: *mut slg_index, rank: c_int, world: c_int, unique_id: *const c_void,
        segs_per_rank: u32) -> *mut slg_shard_group;
    pub fn slg_shard_group_destroy(group: *mut slg_shard_group);
    pub fn slg_batch_run_sharded(batch: *mut slg_batch, group: *mut slg_shard_group, out_doc: *mut u32,
        out_seg: *mut u32, out_score: *mut c_float, out_count: *mut u32) -> c_int;
    pub fn slg_batch_run_sharded_seq(batch: *mut slg_batch, group: *mut slg_shard_group, seq: u64, out_doc: *mut u32,
        out_seg: *mut u32, out_score: *mut c_float, out_count: *mut u32) -> c_int;
    pub fn slg_shard_group_skip_seq(group: *mut slg_shard_group, seq: u64) -> c_int;
    pub fn slg_shard_group_stats(group: *mut slg_shard_group, ms_kernels: *mut f64, ms_gather: *mut f64,
        ms_merge: *mut f64, n_runs: *mut u64) -> c_int;
    pub fn slg_batch_sharded_device_results(batch: *mut slg_batch, d_doc: *mut *mut c_void, d_seg: *mut *mut c_void,
        d_score: *mut *mut c_void, d_count: *mut *mut c_void) -> c_int;
    pub fn slg_batch_fetch_sharded(batch: *mut slg_batch, out_doc: *mut u32, out_seg: *mut u32,
        out_score: *mut c_float, out_count: *mut u32) -> c_int;
    pub fn slg_index_trim_pool(index: *mut slg_index, freed_bytes_or_null: *mut u64) -> c_int;
    pub fn slg_index_set_stream(index: *mut slg_index, hip_stream: *mut c_void) -> c_int;
    // doc filters: accept = !deleted && filter (api/reader.rs:3009-3018)
    pub fn slg_index_add_filter(index: *mut slg_index, seg_bitmaps: *const *const u8) -> c_int;
    pub fn slg_index_add_filter_terms(index: *mut slg_index, term_ids: *const u32, n_terms: u32, pass_if_absent: c_int,
                                      and_bitmaps_or_null: *const *const u8) -> c_int;
    pub fn slg_index_add_filter_range_i64(index: *mut slg_index, seg_columns: *const *const i64, lo: i64, hi: i64) -> c_int;
    pub fn slg_index_add_filter_range_f64(index: *mut slg_index, seg_columns: *const *const f64, lo: f64, hi: f64) -> c_int;
    pub fn slg_index_remove_filter(index: *mut slg_index, filter_id: c_int) -> c_int;
    // sort fields: numeric fast fields as CSR of values per doc (query/sort.rs:300-345); ids are never reused
    pub fn slg_index_add_sort_field_i64(index: *mut slg_index, seg_offsets: *const *const u32,
        seg_values: *const *const i64) -> c_int;
    pub fn slg_index_add_sort_field_f64(index: *mut slg_index, seg_offsets: *const *const u32,
        seg_values: *const *const f64) -> c_int;
    pub fn slg_index_remove_sort_field(index: *mut slg_index, sort_field_id: c_int) -> c_int;
    // one-shot
    pub fn slg_search_batch(index: *mut slg_index, queries: *const slg_query, nq: u32, k: u32,
        strategy: c_int, out_doc: *mut u32, out_seg: *mut u32, out_score: *mut c_float,
        out_count: *mut u32, stats_or_null: *mut slg_stats) -> c_int;
    pub fn slg_search_batch_filtered(index: *mut slg_index, queries: *const slg_query, nq: u32,
        q_filter: *const i32, k: u32, strategy: c_int, out_doc: *mut u32, out_seg: *mut u32,
        out_score: *mut c_float, out_count: *mut u32, stats_or_null: *mut slg_stats) -> c_int;
    // prepared batches (CSR queries; optional score plan and filter per query)
    pub fn slg_batch_prepare(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, k: u32, strategy: c_int) -> *mut slg_batch;
    pub fn slg_batch_prepare_filtered(index: *mut slg_index, nq: u32, q_offsets: *const u32,
        q_term_ids: *const u32, q_weights: *const c_float, q_filter: *const i32, k: u32,
        strategy: c_int) -> *mut slg_batch;
    pub fn slg_batch_prepare_plan(index: *mut slg_index, nq: u32, q_offsets: *const u32,
        q_term_ids: *const u32, q_weights: *const c_float, q_leaf: *const u32, q_plan: *const i32,
        q_tie: *const c_float, q_nleaves: *const u32, q_filter: *const i32, k: u32,
        strategy: c_int) -> *mut slg_batch;
    pub fn slg_batch_prepare_plans(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans_or_null: *const slg_score_plans, q_filter_or_null: *const i32,
        k: u32, strategy: c_int) -> *mut slg_batch;
    pub fn slg_batch_prepare_sorted(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans_or_null: *const slg_score_plans, q_filter_or_null: *const i32,
        sort: *const slg_sort_spec, k: u32, strategy: c_int) -> *mut slg_batch;
    // aggregation columns (ids and lifecycle as sort fields) and aggregation batches (sort NULL: score order)
    pub fn slg_index_add_agg_field_f64(index: *mut slg_index, seg_offsets: *const *const u32,
        seg_values: *const *const f64) -> c_int;
    pub fn slg_index_add_agg_field_i64(index: *mut slg_index, seg_offsets: *const *const u32,
        seg_values: *const *const i64) -> c_int;
    pub fn slg_index_add_agg_field_ord(index: *mut slg_index, seg_offsets: *const *const u32,
        seg_ords: *const *const u32, n_ords: u32) -> c_int;
    pub fn slg_index_remove_agg_field(index: *mut slg_index, agg_field_id: c_int) -> c_int;
    // the value ranks of a column (cardinality and percentiles nodes over a numeric field): the distinct count or < 0
    pub fn slg_index_rank_agg_field(index: *mut slg_index, agg_field_id: c_int) -> i64;
    pub fn slg_batch_prepare_aggs(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans_or_null: *const slg_score_plans, q_filter_or_null: *const i32,
        sort_or_null: *const slg_sort_spec, aggs: *const slg_agg_spec, k: u32, strategy: c_int) -> *mut slg_batch;
    pub fn slg_batch_agg_layout(batch: *const slg_batch, out: *mut slg_agg_layout) -> c_int;
    pub fn slg_batch_fetch_aggs(batch: *mut slg_batch, counts: *mut u64, stats: *mut slg_agg_stats) -> c_int;
    pub fn slg_search_batch_aggs(index: *mut slg_index, queries: *const slg_query, nq: u32,
        plans_or_null: *const slg_score_plans, q_filter_or_null: *const i32, sort_or_null: *const slg_sort_spec,
        aggs: *const slg_agg_spec, k: u32, strategy: c_int, out_doc: *mut u32, out_seg: *mut u32,
        out_score: *mut c_float, out_count: *mut u32, out_matched: *mut u64, counts: *mut u64,
        stats: *mut slg_agg_stats) -> c_int;
    // the value tables (slg_agg_layout.is_stats == 2) of cardinality, percentiles and percentile_ranks nodes
    pub fn slg_batch_fetch_agg_values(batch: *mut slg_batch, values: *mut u64) -> c_int;
    pub fn slg_search_batch_agg_values(index: *mut slg_index, queries: *const slg_query, nq: u32,
        plans_or_null: *const slg_score_plans, q_filter_or_null: *const i32, sort_or_null: *const slg_sort_spec,
        aggs: *const slg_agg_spec, k: u32, strategy: c_int, out_doc: *mut u32, out_seg: *mut u32,
        out_score: *mut c_float, out_count: *mut u32, out_matched: *mut u64, counts: *mut u64,
        stats: *mut slg_agg_stats, values: *mut u64) -> c_int;
    // top_hits: slg_batch_prepare_aggs plus the spec (aggs_or_null: null only when every node is a root); the lists
    // of the last run: doc / seg / score [nq x hit_cells], count [nq x list_cells], status [nq] (1: the CPU path)
    pub fn slg_batch_prepare_top_hits(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans_or_null: *const slg_score_plans, q_filter_or_null: *const i32,
        sort_or_null: *const slg_sort_spec, aggs_or_null: *const slg_agg_spec, top_hits: *const slg_top_hits_spec,
        k: u32, strategy: c_int) -> *mut slg_batch;
    pub fn slg_batch_top_hits_layout(batch: *const slg_batch, out: *mut slg_top_hits_layout) -> c_int;
    pub fn slg_batch_fetch_top_hits(batch: *mut slg_batch, out_doc: *mut u32, out_seg: *mut u32,
        out_score: *mut c_float, out_count: *mut u32, out_status: *mut u32) -> c_int;
    pub fn slg_search_batch_top_hits(index: *mut slg_index, queries: *const slg_query, nq: u32,
        plans_or_null: *const slg_score_plans, q_filter_or_null: *const i32, sort_or_null: *const slg_sort_spec,
        aggs_or_null: *const slg_agg_spec, top_hits: *const slg_top_hits_spec, k: u32, strategy: c_int,
        out_doc: *mut u32, out_seg: *mut u32, out_score: *mut c_float, out_count: *mut u32, out_matched: *mut u64,
        counts: *mut u64, stats: *mut slg_agg_stats, values: *mut u64, th_doc: *mut u32, th_seg: *mut u32,
        th_score: *mut c_float, th_count: *mut u32, th_status: *mut u32) -> c_int;
    // composite: slg_batch_prepare_aggs plus the spec (aggs_or_null may be null); per query an inclusive lower bound
    // in packed key space for the runs that follow (null: from the start); the page of the last run: keys [nq x size]
    // ascending, n_buckets [nq], has_more [nq]
    pub fn slg_batch_prepare_composite(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans_or_null: *const slg_score_plans, q_filter_or_null: *const i32,
        sort_or_null: *const slg_sort_spec, aggs_or_null: *const slg_agg_spec, composite: *const slg_composite_spec,
        k: u32, strategy: c_int) -> *mut slg_batch;
    pub fn slg_batch_composite_layout(batch: *const slg_batch, out: *mut slg_composite_layout) -> c_int;
    pub fn slg_batch_set_composite_after(batch: *mut slg_batch, q_lower_or_null: *const u64) -> c_int;
    pub fn slg_batch_fetch_composite(batch: *mut slg_batch, keys: *mut u64, n_buckets: *mut u32,
        has_more: *mut u32) -> c_int;
    pub fn slg_search_batch_composite(index: *mut slg_index, queries: *const slg_query, nq: u32,
        plans_or_null: *const slg_score_plans, q_filter_or_null: *const i32, sort_or_null: *const slg_sort_spec,
        aggs_or_null: *const slg_agg_spec, composite: *const slg_composite_spec, k: u32, strategy: c_int,
        out_doc: *mut u32, out_seg: *mut u32, out_score: *mut c_float, out_count: *mut u32, out_matched: *mut u64,
        counts: *mut u64, stats: *mut slg_agg_stats, cp_keys: *mut u64, cp_n_buckets: *mut u32,
        cp_has_more: *mut u32) -> c_int;
    // significant_terms / rare_terms: slg_batch_prepare_aggs plus the spec (aggs_or_null may be null); the buckets of
    // the last run in the response's order: [nq x rows] per row array, [nq x n_nodes] per node array (any may be null)
    pub fn slg_batch_prepare_term_buckets(index: *mut slg_index, nq: u32, q_offsets: *const u32,
        q_term_ids: *const u32, q_weights: *const c_float, plans_or_null: *const slg_score_plans,
        q_filter_or_null: *const i32, sort_or_null: *const slg_sort_spec, aggs_or_null: *const slg_agg_spec,
        spec: *const slg_term_bucket_spec, k: u32, strategy: c_int) -> *mut slg_batch;
    pub fn slg_batch_term_buckets_layout(batch: *const slg_batch, out: *mut slg_term_bucket_layout) -> c_int;
    pub fn slg_batch_fetch_term_buckets(batch: *mut slg_batch, ords: *mut u32, doc_counts: *mut u64,
        bg_counts: *mut u64, score_bits: *mut u64, n_buckets: *mut u32, node_doc_count: *mut u64,
        node_bg_count: *mut u64) -> c_int;
    pub fn slg_search_batch_term_buckets(index: *mut slg_index, queries: *const slg_query, nq: u32,
        plans_or_null: *const slg_score_plans, q_filter_or_null: *const i32, sort_or_null: *const slg_sort_spec,
        aggs_or_null: *const slg_agg_spec, spec: *const slg_term_bucket_spec, k: u32, strategy: c_int,
        out_doc: *mut u32, out_seg: *mut u32, out_score: *mut c_float, out_count: *mut u32, out_matched: *mut u64,
        counts: *mut u64, stats: *mut slg_agg_stats, tb_ords: *mut u32, tb_doc_counts: *mut u64,
        tb_bg_counts: *mut u64, tb_score_bits: *mut u64, tb_n_buckets: *mut u32, tb_node_doc_count: *mut u64,
        tb_node_bg_count: *mut u64) -> c_int;
    pub fn slg_batch_matched_counts(batch: *mut slg_batch, out_matched: *mut u64) -> c_int;
    pub fn slg_search_batch_sorted(index: *mut slg_index, queries: *const slg_query, nq: u32,
        plans_or_null: *const slg_score_plans, q_filter_or_null: *const i32, sort: *const slg_sort_spec, k: u32,
        strategy: c_int, out_doc: *mut u32, out_seg: *mut u32, out_score: *mut c_float, out_count: *mut u32,
        out_matched: *mut u64) -> c_int;
    // cursor pagination: the top k strictly after each query's cursor (sort NULL: score order)
    pub fn slg_batch_prepare_after(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans_or_null: *const slg_score_plans, q_filter_or_null: *const i32,
        sort_or_null: *const slg_sort_spec, q_cursor: *const slg_sort_cursor, k: u32, strategy: c_int) -> *mut slg_batch;
    pub fn slg_batch_cursor_seen(batch: *mut slg_batch, out_seen: *mut u8) -> c_int;
    pub fn slg_search_batch_after(index: *mut slg_index, queries: *const slg_query, nq: u32,
        plans_or_null: *const slg_score_plans, q_filter_or_null: *const i32, sort_or_null: *const slg_sort_spec,
        q_cursor: *const slg_sort_cursor, k: u32, strategy: c_int, out_doc: *mut u32, out_seg: *mut u32,
        out_score: *mut c_float, out_count: *mut u32, out_matched: *mut u64, out_seen: *mut u8) -> c_int;
    pub fn slg_batch_set_stream(batch: *mut slg_batch, hip_stream: *mut c_void) -> c_int;
    pub fn slg_batch_run(batch: *mut slg_batch) -> c_int;
    pub fn slg_batch_sync(batch: *mut slg_batch) -> c_int;
    pub fn slg_batch_fetch(batch: *mut slg_batch, out_doc: *mut u32, out_seg: *mut u32, out_score: *mut c_float,
        out_count: *mut u32, stats_or_null: *mut slg_stats) -> c_int;
    pub fn slg_batch_device_results(batch: *mut slg_batch, d_doc: *mut *mut c_void, d_seg: *mut *mut c_void,
        d_score: *mut *mut c_void, d_count: *mut *mut c_void) -> c_int;
    pub fn slg_batch_device_result_block(batch: *mut slg_batch, d_block: *mut *mut c_void, n_bytes: *mut u64) -> c_int;
    pub fn slg_batch_info(batch: *const slg_batch, n_postings: *mut u64, n_slices: *mut u32, algorithmic_bytes: *mut u64) -> c_int;
    pub fn slg_batch_skip_counts(batch: *mut slg_batch, probed_postings: *mut u64, skipped_postings: *mut u64) -> c_int;
    pub fn slg_batch_destroy(batch: *mut slg_batch);
    // multi-GPU merge of per-shard result blocks, profiling, rerank
    pub fn slg_merge_shards_device(index: *mut slg_index, n_shards: u32, nq: u32, k: u32,
        d_doc: *const u32, d_seg: *const u32, d_score: *const c_float, d_count: *const u32, seg_stride: u32,
        d_out_doc: *mut u32, d_out_seg: *mut u32, d_out_score: *mut c_float, d_out_count: *mut u32) -> c_int;
    pub fn slg_profile_enable(index: *mut slg_index, on: c_int) -> c_int;
    pub fn slg_profile_read(index: *mut slg_index, n_launches: *mut u32, total_ms: *mut c_float) -> c_int;
    pub fn slg_rerank_batch(index: *mut slg_index, nq: u32, qvecs: *const c_float, alpha: *const c_float,
        cand_doc: *const u32, cand_seg: *const u32, cand_bm25: *const c_float, cand_count: *const u32,
        max_cand: u32, k_out: u32, out_doc: *mut u32, out_seg: *mut u32, out_score: *mut c_float,
        out_vec_score: *mut c_float, out_count: *mut u32) -> c_int;
    pub fn slg_rerank_batch_device(index: *mut slg_index, nq: u32, d_qvecs: *const c_float, d_alpha: *const c_float,
        d_cand_doc: *const u32, d_cand_seg: *const u32, d_cand_bm25: *const c_float, d_cand_count: *const u32,
        max_cand: u32, k_out: u32, d_out_doc: *mut u32, d_out_seg: *mut u32, d_out_score: *mut c_float,
        d_out_vec_score: *mut c_float, d_out_count: *mut u32) -> c_int;
    pub fn slg_batch_rerank_device(batch: *mut slg_batch, n_clauses: u32, d_qvecs: *const c_float, d_alpha: *const c_float,
        d_boost: *const c_float, k_out: u32, d_out_doc: *mut u32, d_out_seg: *mut u32, d_out_score: *mut c_float,
        d_out_vec_score: *mut c_float, d_out_count: *mut u32) -> c_int;
    pub fn slg_index_add_vector_field(index: *mut slg_index, per_segment: *const slg_vector_field_desc, n_segs: u32) -> c_int;
    pub fn slg_rerank_fields_batch(index: *mut slg_index, nq: u32, n_clauses: u32, clause_field: *const u32,
        qvecs: *const c_float, alpha: *const c_float, boost: *const c_float, cand_doc: *const u32, cand_seg: *const u32,
        cand_bm25: *const c_float, cand_count: *const u32, max_cand: u32, k_out: u32, out_doc: *mut u32,
        out_seg: *mut u32, out_score: *mut c_float, out_vec_score: *mut c_float, out_count: *mut u32) -> c_int;
    pub fn slg_rerank_fields_batch_device(index: *mut slg_index, nq: u32, n_clauses: u32, clause_field: *const u32,
        d_qvecs: *const c_float, d_alpha: *const c_float, d_boost: *const c_float, d_cand_doc: *const u32,
        d_cand_seg: *const u32, d_cand_bm25: *const c_float, d_cand_count: *const u32, max_cand: u32, k_out: u32,
        d_out_doc: *mut u32, d_out_seg: *mut u32, d_out_score: *mut c_float, d_out_vec_score: *mut c_float,
        d_out_count: *mut u32) -> c_int;
    pub fn slg_rerank_multi_batch(index: *mut slg_index, nq: u32, n_clauses: u32, qvecs: *const c_float,
        alpha: *const c_float, boost: *const c_float, cand_doc: *const u32, cand_seg: *const u32,
        cand_bm25: *const c_float, cand_count: *const u32, max_cand: u32, k_out: u32, out_doc: *mut u32,
        out_seg: *mut u32, out_score: *mut c_float, out_vec_score: *mut c_float, out_count: *mut u32) -> c_int;
    pub fn slg_rerank_multi_batch_device(index: *mut slg_index, nq: u32, n_clauses: u32, d_qvecs: *const c_float,
        d_alpha: *const c_float, d_boost: *const c_float, d_cand_doc: *const u32, d_cand_seg: *const u32,
        d_cand_bm25: *const c_float, d_cand_count: *const u32, max_cand: u32, k_out: u32, d_out_doc: *mut u32,
        d_out_seg: *mut u32, d_out_score: *mut c_float, d_out_vec_score: *mut c_float, d_out_count: *mut u32) -> c_int;
    pub fn slg_vector_search_batch(index: *mut slg_index, nq: u32, n_clauses: u32, clause_field: *const u32,
        qvecs: *const c_float, alpha: *const c_float, boost: *const c_float, q_filter: *const i32, cand_size: u32,
        k_out: u32, out_doc: *mut u32, out_seg: *mut u32, out_score: *mut c_float, out_vec_score: *mut c_float,
        out_count: *mut u32, out_total: *mut u64) -> c_int;
    pub fn slg_vector_search_batch_device(index: *mut slg_index, nq: u32, n_clauses: u32, clause_field: *const u32,
        d_qvecs: *const c_float, d_alpha: *const c_float, d_boost: *const c_float, d_q_filter: *const i32,
        cand_size: u32, k_out: u32, d_out_doc: *mut u32, d_out_seg: *mut u32, d_out_score: *mut c_float,
        d_out_vec_score: *mut c_float, d_out_count: *mut u32, d_out_total: *mut u64) -> c_int;
    // two-pass vector search: a bf16 copy of a field's stores, a first pass over it, exact scores for `refine` docs
    pub fn slg_index_quantize_vector_field(index: *mut slg_index, field: u32) -> c_int;
    pub fn slg_index_fetch_vector_copy(index: *mut slg_index, field: u32, seg: u32, out_u16: *mut u16,
        out_norm: *mut c_float, rows_cap: u32) -> c_int;
    pub fn slg_vector_search_batch_approx(index: *mut slg_index, nq: u32, n_clauses: u32, clause_field: *const u32,
        qvecs: *const c_float, alpha: *const c_float, boost: *const c_float, q_filter: *const i32, cand_size: u32,
        refine: u32, k_out: u32, out_doc: *mut u32, out_seg: *mut u32, out_score: *mut c_float,
        out_vec_score: *mut c_float, out_count: *mut u32, out_total: *mut u64) -> c_int;
    pub fn slg_vector_search_batch_approx_device(index: *mut slg_index, nq: u32, n_clauses: u32,
        clause_field: *const u32, d_qvecs: *const c_float, d_alpha: *const c_float, d_boost: *const c_float,
        d_q_filter: *const i32, cand_size: u32, refine: u32, k_out: u32, d_out_doc: *mut u32, d_out_seg: *mut u32,
        d_out_score: *mut c_float, d_out_vec_score: *mut c_float, d_out_count: *mut u32,
        d_out_total: *mut u64) -> c_int;
    // IVF vector search: lists around caller-supplied centroids per (field, segment), the nprobe nearest are scanned
    pub fn slg_index_cluster_vector_field(index: *mut slg_index, field: u32,
        per_segment: *const slg_vector_lists_desc, n_segs: u32) -> c_int;
    pub fn slg_index_fetch_vector_lists(index: *mut slg_index, field: u32, seg: u32, out_list_begin: *mut u32,
        out_docs: *mut u32, out_centroids: *mut c_float, lists_cap: u32, docs_cap: u32) -> c_int;
    // Lloyd steps over the f32 store on the device, then the lists of the trained centroids (out_stats may be null)
    pub fn slg_index_train_vector_field(index: *mut slg_index, field: u32,
        per_segment: *const slg_vector_train_desc, n_segs: u32, out_stats: *mut slg_vector_train_stats) -> c_int;
    pub fn slg_vector_search_batch_ivf(index: *mut slg_index, nq: u32, n_clauses: u32, clause_field: *const u32,
        qvecs: *const c_float, alpha: *const c_float, boost: *const c_float, q_filter: *const i32, cand_size: u32,
        nprobe: u32, k_out: u32, out_doc: *mut u32, out_seg: *mut u32, out_score: *mut c_float,
        out_vec_score: *mut c_float, out_count: *mut u32, out_total: *mut u64) -> c_int;
    pub fn slg_vector_search_batch_ivf_device(index: *mut slg_index, nq: u32, n_clauses: u32,
        clause_field: *const u32, d_qvecs: *const c_float, d_alpha: *const c_float, d_boost: *const c_float,
        d_q_filter: *const i32, cand_size: u32, nprobe: u32, k_out: u32, d_out_doc: *mut u32, d_out_seg: *mut u32,
        d_out_score: *mut c_float, d_out_vec_score: *mut c_float, d_out_count: *mut u32,
        d_out_total: *mut u64) -> c_int;
    // hybrid text + vector search (merge_vector_hits): prepare, run (slg_batch_run), then the vector side
    pub fn slg_batch_prepare_hybrid(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32, k: u32,
        strategy: c_int) -> *mut slg_batch;
    pub fn slg_batch_hybrid_device(batch: *mut slg_batch, n_clauses: u32, clause_field: *const u32,
        d_qvecs: *const c_float, d_alpha: *const c_float, d_boost: *const c_float, cand_size: u32, k_out: u32,
        d_out_doc: *mut u32, d_out_seg: *mut u32, d_out_score: *mut c_float, d_out_vec_score: *mut c_float,
        d_out_count: *mut u32, d_out_total: *mut u64) -> c_int;
    pub fn slg_search_batch_hybrid(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32, k: u32, strategy: c_int,
        n_clauses: u32, clause_field: *const u32, qvecs: *const c_float, alpha: *const c_float,
        boost: *const c_float, cand_size: u32, k_out: u32, out_doc: *mut u32, out_seg: *mut u32,
        out_score: *mut c_float, out_vec_score: *mut c_float, out_count: *mut u32, out_total: *mut u64) -> c_int;
    // query rescore (SearchRequest::rescore): slg_batch_prepare_plans plus the spec; the rows are the rescored ones
    pub fn slg_batch_prepare_rescore(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32,
        rescore: *const slg_rescore_spec, k: u32, strategy: c_int) -> *mut slg_batch;
    pub fn slg_batch_fetch_rescore(batch: *mut slg_batch, out_first_score: *mut c_float,
        out_rescore_score: *mut c_float, out_rescored: *mut u32) -> c_int;
    pub fn slg_search_batch_rescore(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32,
        rescore: *const slg_rescore_spec, k: u32, strategy: c_int, out_doc: *mut u32, out_seg: *mut u32,
        out_score: *mut c_float, out_count: *mut u32, out_first_score: *mut c_float,
        out_rescore_score: *mut c_float, out_rescored: *mut u32) -> c_int;
    // boolean queries (must / should / must_not groups of terms): slg_batch_prepare_plans or _sorted plus the spec
    pub fn slg_batch_prepare_bool(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32,
        sort: *const slg_sort_spec, spec: *const slg_bool_spec, k: u32, strategy: c_int) -> *mut slg_batch;
    pub fn slg_search_batch_bool(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32,
        sort: *const slg_sort_spec, spec: *const slg_bool_spec, k: u32, strategy: c_int, out_doc: *mut u32,
        out_seg: *mut u32, out_score: *mut c_float, out_count: *mut u32, stats: *mut slg_stats,
        out_matched: *mut u64) -> c_int;
    // nested boolean matchers (a tree of bool / dis_max / query string nodes over term groups and filter ids):
    // the argument shape of the two bool calls.  The shim does not route requests to them yet.
    pub fn slg_batch_prepare_bool_tree(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32,
        sort: *const slg_sort_spec, spec: *const slg_bool_tree_spec, k: u32, strategy: c_int) -> *mut slg_batch;
    pub fn slg_search_batch_bool_tree(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32,
        sort: *const slg_sort_spec, spec: *const slg_bool_tree_spec, k: u32, strategy: c_int, out_doc: *mut u32,
        out_seg: *mut u32, out_score: *mut c_float, out_count: *mut u32, stats: *mut slg_stats,
        out_matched: *mut u64) -> c_int;
    // phrase queries: positions per segment, then slg_batch_prepare_bool plus the phrase spec (bool_spec may be null)
    pub fn slg_index_set_positions(index: *mut slg_index, seg: u32, pos_offsets: *const u64, positions: *const u32) -> c_int;
    // term expansion: a dictionary per segment, then fuzzy / prefix / wildcard requests -> rows of term ids
    pub fn slg_index_set_terms(index: *mut slg_index, seg: u32, key_bytes: *const c_char, key_offsets: *const u32) -> c_int;
    pub fn slg_expand_batch(index: *mut slg_index, reqs: *const slg_expand_req, n_reqs: u32, out_offsets: *mut u32,
        key_capacity: u32, out_term_ids: *mut u32, out_distance: *mut u8) -> c_int;
    // diagnostic only (the timing tool's split of the last call on this thread into scan and merge): not routed
    pub fn slg_expand_phase_ms(index: *mut slg_index, scan_ms: *mut f64, merge_ms: *mut f64) -> c_int;
    // the completion suggester (SearchRequest.suggest): declared, not routed yet
    pub fn slg_suggest_batch(index: *mut slg_index, reqs: *const slg_suggest_req, n_reqs: u32, out_offsets: *mut u32,
        option_capacity: u32, out_score: *mut c_float, out_doc_freq: *mut u64, out_text_offsets: *mut u32,
        text_capacity: u32, out_text: *mut c_char) -> c_int;
    pub fn slg_suggest_phase_ms(index: *mut slg_index, device_ms: *mut f64, copy_ms: *mut f64) -> c_int;
    // highlighting (SearchRequest.highlight / highlight_field) over registered texts: declared, not routed yet
    // (INTEGRATION.md says how materialize_hit would use it)
    pub fn slg_index_add_text_field(index: *mut slg_index, seg_offsets: *const *const u64,
        seg_bytes: *const *const u8) -> c_int;
    pub fn slg_index_remove_text_field(index: *mut slg_index, text_field_id: c_int) -> c_int;
    pub fn slg_highlight_batch(index: *mut slg_index, n_queries: u32, hit_offsets: *const u32, hit_seg: *const u32,
        hit_doc: *const u32, spec_offsets: *const u32, specs: *const slg_hl_spec, out: *mut slg_hl_out) -> c_int;
    pub fn slg_batch_highlight(batch: *mut slg_batch, spec_offsets: *const u32, specs: *const slg_hl_spec,
        out: *mut slg_hl_out) -> c_int;
    pub fn slg_highlight_phase_ms(index: *mut slg_index, count_ms: *mut f64, emit_ms: *mut f64) -> c_int;
    // explain (SearchRequest.explain) behind a batch that has run: declared, not routed yet (INTEGRATION.md says
    // how the request path would use it)
    pub fn slg_batch_explain(batch: *mut slg_batch, rows: u32, out: *const slg_explain_out) -> c_int;
    pub fn slg_batch_prepare_phrase(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32,
        sort: *const slg_sort_spec, bool_spec: *const slg_bool_spec, phrases: *const slg_phrase_spec, k: u32,
        strategy: c_int) -> *mut slg_batch;
    pub fn slg_search_batch_phrase(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32,
        sort: *const slg_sort_spec, bool_spec: *const slg_bool_spec, phrases: *const slg_phrase_spec, k: u32,
        strategy: c_int, out_doc: *mut u32, out_seg: *mut u32, out_score: *mut c_float, out_count: *mut u32,
        stats: *mut slg_stats, out_matched: *mut u64) -> c_int;
    // function_score at the root (weight, field_value_factor, decay, min_score): slg_batch_prepare_plans or _sorted
    // plus the spec; columns are those of slg_index_add_agg_field_f64 / _i64
    pub fn slg_batch_prepare_fscore(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32,
        sort: *const slg_sort_spec, spec: *const slg_fscore_spec, k: u32, strategy: c_int) -> *mut slg_batch;
    // script_score at the root (arithmetic over _score, constants and numeric columns), alone or chained with a
    // function_score stage (order: SLG_SCRIPT_OUTER = script_score{function_score}, _INNER = the other nesting)
    pub fn slg_batch_prepare_script(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32,
        sort: *const slg_sort_spec, script: *const slg_script_spec, fscore: *const slg_fscore_spec, order: c_int,
        k: u32, strategy: c_int) -> *mut slg_batch;
    pub fn slg_batch_script_info(batch: *const slg_batch, out_queries_with_work: *mut u32, out_max_depth: *mut u32) -> c_int;
    pub fn slg_search_batch_script(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32,
        sort: *const slg_sort_spec, script: *const slg_script_spec, fscore: *const slg_fscore_spec, order: c_int,
        k: u32, strategy: c_int, out_doc: *mut u32, out_seg: *mut u32, out_score: *mut c_float, out_count: *mut u32,
        stats: *mut slg_stats, out_matched: *mut u64) -> c_int;
    pub fn slg_index_add_filter_trees(index: *mut slg_index, trees: *const slg_filter_tree, n_trees: u32,
        out_ids: *mut i32) -> c_int;
    pub fn slg_index_fetch_filter(index: *mut slg_index, filter_id: c_int, seg: u32, out_pass: *mut u8) -> c_int;
    pub fn slg_index_add_nested_path(index: *mut slg_index, parent_path_id: c_int, seg_counts: *const *const u32,
        seg_parent_offsets: *const *const u32, seg_parents: *const *const u32) -> c_int;
    pub fn slg_index_remove_nested_path(index: *mut slg_index, path_id: c_int) -> c_int;
    pub fn slg_index_add_nested_field_f64(index: *mut slg_index, path_id: c_int, seg_doc_offsets: *const *const u32,
        seg_object_offsets: *const *const u32, seg_values: *const *const f64) -> c_int;
    pub fn slg_index_add_nested_field_i64(index: *mut slg_index, path_id: c_int, seg_doc_offsets: *const *const u32,
        seg_object_offsets: *const *const u32, seg_values: *const *const i64) -> c_int;
    pub fn slg_index_add_nested_field_ord(index: *mut slg_index, path_id: c_int, seg_doc_offsets: *const *const u32,
        seg_object_offsets: *const *const u32, seg_ords: *const *const u32, n_ords: u32) -> c_int;
    pub fn slg_index_remove_nested_field(index: *mut slg_index, nested_field_id: c_int) -> c_int;
    pub fn slg_index_add_nested_filter_trees(index: *mut slg_index, trees: *const slg_nested_filter_tree, n_trees: u32,
        out_ids: *mut i32) -> c_int;
    // diagnostic only (the planner's champion table of a segment, [n_terms * 68]): not routed
    pub fn slg_index_fetch_champions(index: *const slg_index, seg: u32, out: *mut c_float) -> c_int;
    pub fn slg_batch_fscore_info(batch: *const slg_batch, out_variant: *mut u32, out_queries_with_work: *mut u32) -> c_int;
    pub fn slg_search_batch_fscore(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32,
        sort: *const slg_sort_spec, spec: *const slg_fscore_spec, k: u32, strategy: c_int, out_doc: *mut u32,
        out_seg: *mut u32, out_score: *mut c_float, out_count: *mut u32, stats: *mut slg_stats,
        out_matched: *mut u64) -> c_int;
    // scan batches (match_all, constant_score, rank_feature at the root): no query arrays; sort and aggs as in
    // slg_batch_prepare_aggs, both may be null; run / fetch / matched counts / aggregation tables as for any batch.
    // Bound, not routed: reader_gpu.patch.rs sends no request here yet
    pub fn slg_batch_prepare_scan(index: *mut slg_index, nq: u32, spec: *const slg_scan_spec, q_filter: *const i32,
        sort: *const slg_sort_spec, aggs: *const slg_agg_spec, k: u32) -> *mut slg_batch;
    pub fn slg_batch_scan_info(batch: *const slg_batch, out_variant: *mut u32, out_slices: *mut u32,
        out_slice_docs: *mut u32) -> c_int;
    pub fn slg_search_batch_scan(index: *mut slg_index, nq: u32, spec: *const slg_scan_spec, q_filter: *const i32,
        sort: *const slg_sort_spec, aggs: *const slg_agg_spec, k: u32, out_doc: *mut u32, out_seg: *mut u32,
        out_score: *mut c_float, out_count: *mut u32, out_matched: *mut u64, counts: *mut u64,
        stats: *mut slg_agg_stats, values: *mut u64) -> c_int;
    // field collapsing: slg_batch_prepare_plans, _sorted or _after plus the spec; the rows stay as they are, the
    // groups and inner hits of each query's rows come from slg_batch_fetch_collapse
    pub fn slg_batch_prepare_collapse(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32,
        sort: *const slg_sort_spec, q_cursor: *const slg_sort_cursor, collapse: *const slg_collapse_spec, k: u32,
        strategy: c_int) -> *mut slg_batch;
    pub fn slg_batch_fetch_collapse(batch: *mut slg_batch, n_groups: *mut u32, total_groups: *mut u32,
        status: *mut u32, group_row: *mut u32, group_ord: *mut u32, group_size: *mut u32, group_doc: *mut u32,
        group_seg: *mut u32, group_score: *mut c_float, inner_count: *mut u32, inner_row: *mut u32,
        inner_doc: *mut u32, inner_seg: *mut u32, inner_score: *mut c_float) -> c_int;
    pub fn slg_search_batch_collapse(index: *mut slg_index, nq: u32, q_offsets: *const u32, q_term_ids: *const u32,
        q_weights: *const c_float, plans: *const slg_score_plans, q_filter: *const i32,
        sort: *const slg_sort_spec, q_cursor: *const slg_sort_cursor, collapse: *const slg_collapse_spec, k: u32,
        strategy: c_int, out_doc: *mut u32, out_seg: *mut u32, out_score: *mut c_float, out_count: *mut u32,
        n_groups: *mut u32, total_groups: *mut u32, status: *mut u32, group_row: *mut u32, group_ord: *mut u32,
        group_size: *mut u32, group_doc: *mut u32, group_seg: *mut u32, group_score: *mut c_float,
        inner_count: *mut u32, inner_row: *mut u32, inner_doc: *mut u32, inner_seg: *mut u32,
        inner_score: *mut c_float) -> c_int;
    pub fn slg_batch_prepare_request(index: *mut slg_index, req: *const slg_request) -> *mut slg_batch;
}
pub const SLG_MAX_COLLAPSE_ROWS: u32 = 4096;
pub const SLG_MAX_INNER_HITS: u32 = 64;
pub const SLG_MAX_PHRASE_TERMS: u32 = 8;
pub const SLG_MAX_PHRASE_VARIANTS: u32 = 8;
pub const SLG_MAX_PHRASE_QUERY_TERMS: u32 = 64;
pub const SLG_MAX_PHRASE_SLOP: u32 = 2147483639;
pub const SLG_BOOL_MUST: i32 = 0;
pub const SLG_BOOL_SHOULD: i32 = 1;
pub const SLG_BOOL_MUST_NOT: i32 = 2;
pub const SLG_MAX_BOOL_GROUPS: u32 = 32;
pub const SLG_MAX_BOOL_TERMS: u32 = 64;
pub const SLG_MAX_BOOL_TREE_LEAVES: u32 = 32;
pub const SLG_MAX_BOOL_TREE_NODES: u32 = 32;
pub const SLG_MAX_FSCORE_FUNCS: u32 = 8;
pub const SLG_FSCORE_WEIGHT: i32 = 0;
pub const SLG_FSCORE_FIELD_VALUE_FACTOR: i32 = 1;
pub const SLG_FSCORE_DECAY: i32 = 2;
pub const SLG_FSCORE_MOD_NONE: i32 = 0;
pub const SLG_FSCORE_MOD_LOG: i32 = 1;
pub const SLG_FSCORE_MOD_LOG1P: i32 = 2;
pub const SLG_FSCORE_MOD_LOG2P: i32 = 3;
pub const SLG_FSCORE_MOD_SQRT: i32 = 4;
pub const SLG_FSCORE_MOD_RECIPROCAL: i32 = 5;
pub const SLG_FSCORE_DECAY_EXP: i32 = 0;
pub const SLG_FSCORE_DECAY_GAUSS: i32 = 1;
pub const SLG_FSCORE_DECAY_LINEAR: i32 = 2;
pub const SLG_FSCORE_MODE_SUM: i32 = 0;
pub const SLG_FSCORE_MODE_MULTIPLY: i32 = 1;
pub const SLG_FSCORE_MODE_MAX: i32 = 2;
pub const SLG_FSCORE_MODE_MIN: i32 = 3;
pub const SLG_FSCORE_MODE_AVG: i32 = 4;
pub const SLG_FSCORE_BOOST_MULTIPLY: i32 = 0;
pub const SLG_FSCORE_BOOST_SUM: i32 = 1;
pub const SLG_FSCORE_BOOST_REPLACE: i32 = 2;
pub const SLG_FSCORE_BOOST_MAX: i32 = 3;
pub const SLG_FSCORE_BOOST_MIN: i32 = 4;
pub const SLG_FSCORE_HAS_MAX_BOOST: u32 = 1;
pub const SLG_FSCORE_HAS_MIN_SCORE: u32 = 2;
pub const SLG_MAX_SCRIPT_INSTRS: u32 = 64;
pub const SLG_MAX_SCRIPT_DEPTH: u32 = 8;
pub const SLG_MAX_SCRIPT_FIELDS: u32 = 8;
pub const SLG_SCRIPT_PUSH_CONST: i32 = 0;
pub const SLG_SCRIPT_PUSH_FIELD: i32 = 1;
pub const SLG_SCRIPT_PUSH_SCORE: i32 = 2;
pub const SLG_SCRIPT_ADD: i32 = 3;
pub const SLG_SCRIPT_SUB: i32 = 4;
pub const SLG_SCRIPT_MUL: i32 = 5;
pub const SLG_SCRIPT_DIV: i32 = 6;
pub const SLG_SCRIPT_NEG: i32 = 7;
pub const SLG_SCRIPT_OUTER: i32 = 0;
pub const SLG_SCRIPT_INNER: i32 = 1;
pub const SLG_FILTER_KEYWORD_IN: i32 = 0;
pub const SLG_FILTER_RANGE_F64: i32 = 1;
pub const SLG_FILTER_RANGE_I64: i32 = 2;
pub const SLG_FILTER_ID: i32 = 3;
pub const SLG_FILTER_AND: i32 = 4;
pub const SLG_FILTER_OR: i32 = 5;
pub const SLG_FILTER_NOT: i32 = 6;
pub const SLG_MAX_FILTER_NODES: u32 = 64;
pub const SLG_MAX_FILTER_DEPTH: u32 = 16;
pub const SLG_MAX_FILTER_TREES: u32 = 64;
pub const SLG_FILTER_NESTED: i32 = 7;
pub const SLG_MAX_NESTED_SCOPES: u32 = 16;
pub const SLG_MAX_NESTED_DEPTH: u32 = 4;
pub const SLG_RESCORE_TOTAL: i32 = 0;
pub const SLG_RESCORE_MULTIPLY: i32 = 1;
pub const SLG_RESCORE_SUM: i32 = 2;
pub const SLG_RESCORE_MAX: i32 = 3;
pub const SLG_RESCORE_MIN: i32 = 4;
pub const SLG_MAX_RESCORE_WINDOW: u32 = 1024;
pub const SLG_OWN_STREAM: *mut c_void = usize::MAX as *mut c_void;
pub const SLG_NO_TERM: u32 = 0xFFFF_FFFF;
pub const SLG_METRIC_COSINE: i32 = 0;
pub const SLG_METRIC_L2: i32 = 1;
pub const SLG_STRATEGY_BM25: c_int = 0;
pub const SLG_STRATEGY_WAND: c_int = 1;
pub const SLG_STRATEGY_BMW: c_int = 2;
pub const SLG_PLAN_SUM: i32 = 0;
pub const SLG_PLAN_DISMAX: i32 = 1;
pub const SLG_PLAN_LEAF: i32 = 2;
pub const SLG_MAX_PLAN_DEPTH: usize = 4;
pub const SLG_MAX_SORT_PARTS: usize = 4;
pub const SLG_SORT_SCORE: i32 = -1;
pub const SLG_ORDER_ASC: i32 = 0;
pub const SLG_ORDER_DESC: i32 = 1;
