/*
 * searchlite_gpu.h — C ABI of the MI355X (gfx950) batched BM25 top-k scorer + vector rerank.
 *
 * This is the drop-in boundary for ONE path of davidkelley/searchlite: the per-segment
 * top-k scorer that `IndexReader::search_segment` calls
 * (searchlite-core/src/api/reader.rs:3075-3099 ->
 *  execute_top_k_with_stats_and_mode_internal, searchlite-core/src/query/wand.rs:398-412),
 * the cross-segment merge that follows it (api/reader.rs:2776-2778, query/sort.rs:80-93),
 * and the rerank slot `gpu::rerank` (searchlite-core/src/gpu/rerank.rs:3) behind the
 * `gpu` cargo feature (searchlite-core/src/lib.rs:11-12, Cargo.toml:13).
 *
 * Conventions follow searchlite's own C FFI (searchlite-ffi/searchlite.h:12-18,
 * searchlite-ffi/src/lib.rs:24-43,58-91): opaque handles, NULL / negative int on error,
 * caller-owned output buffers, no exceptions or panics across the boundary, and a
 * thread-local last-error string.  Plain pointers and sizes only.
 *
 * Eligibility (the caller keeps every other request shape on searchlite's CPU scorer;
 * SURVEY.md section 8b): ScoreMode::Score, sort = _score desc, no collector/aggs, no
 * score_adjust/explain, matcher = pure disjunction; filters as doc bitmaps
 * (slg_index_add_filter*: accept() = !is_deleted(doc) && filter(doc)); ScorePlan = any tree of Sum /
 * DisMax nodes up to SLG_MAX_PLAN_DEPTH levels above its leaves, each leaf the sum of one or more
 * scored terms (slg_batch_prepare_plans; the default is leaf i == query term i, summed);
 * k = limit + 1 up to 20 001; up to 32 scored terms per query and segment.  Field sorts (slg_batch_prepare_sorted):
 * up to SLG_MAX_SORT_PARTS parts of numeric fast fields (i64 / f64) and _score, any order; keyword parts stay
 * on the CPU.  A cursor (the next page, slg_batch_prepare_after) in score order or in a device-eligible field
 * sort; not in sharded runs or the coalescer.  Aggregations (slg_batch_prepare_aggs): terms, histogram, range,
 * stats, cardinality, percentiles and percentile_ranks over registered columns, two levels, in score order or a field sort; not with a cursor, not on hybrid,
 * vector-only, sharded or coalesced batches.  Query rescore (slg_batch_prepare_rescore): a second BM25 query with
 * a flat Sum / DisMax plan over a window of up to SLG_MAX_RESCORE_WINDOW first-pass rows, every score_mode; in
 * score order only, not on sorted, cursor, hybrid, vector-only, aggregation, sharded or coalesced batches.
 * Boolean queries (slg_batch_prepare_bool): must / should / must_not groups of terms and minimum_should_match
 * over up to SLG_MAX_BOOL_GROUPS groups, in score order or a field sort; not on
 * cursor, hybrid, aggregation, rescore, sharded or coalesced batches.  Nested boolean matchers
 * (slg_batch_prepare_bool_tree): a tree of bool / dis_max / query string / match_all nodes over term groups and
 * registered filters (a bool's own filter list), up to SLG_MAX_BOOL_TREE_LEAVES leaves and
 * SLG_MAX_BOOL_TREE_NODES nodes, where a bool batch runs; phrase leaves in a tree stay on the CPU.  Phrase queries
 * (slg_index_set_positions, slg_batch_prepare_phrase): phrase groups with a slop and per-field variants beside
 * the term groups of a bool batch, under the same limits; one term per phrase position (no position
 * alternatives), not in rescore queries.  Field collapsing (slg_batch_prepare_collapse): one hit per ordinal of a
 * keyword column over the k <= SLG_MAX_COLLAPSE_ROWS rows of a plain, sorted or cursor batch, with up to
 * SLG_MAX_INNER_HITS inner hits per group; not with aggregations, rescore, bool, phrase, function_score, hybrid or
 * vector-only batches, sharded or coalesced.  Term expansion (slg_index_set_terms, slg_expand_batch): the fuzzy
 * option of a request and Prefix / Wildcard / Regex nodes are expanded against the segments' term dictionaries on
 * the device into ordinary slg_query terms, keys in the reference's order; terms or patterns of up to
 * SLG_MAX_EXPAND_CHARS chars, max_expansions up to SLG_MAX_EXPANSIONS; a regex as a byte-level DFA of up to
 * SLG_MAX_REGEX_STATES states (no Unicode perl classes, flags or case folding).  Unscored groups, a query that
 * folds to more than SLG_MAX_QUERY_TERMS terms, and expansion inside sharded or coalesced paths stay on the CPU.
 * The completion suggester (slg_suggest_batch): SuggestRequest::Completion, plain prefix or fuzzy, against the
 * same dictionaries and their doc frequencies; scan, merge across segments, scores and the best `size` on the
 * device; terms of up to SLG_MAX_EXPAND_CHARS chars, a fuzzy request's size up to SLG_MAX_SUGGEST_CANDIDATES.  The
 * analysis of the prefix, and suggest through the coalescer or shard groups, stay with the caller.
 * Highlighting (slg_index_add_text_field, slg_highlight_batch, slg_batch_highlight): SearchRequest.highlight and
 * highlight_field over stored texts registered with the index; the fragments of every (hit, field) with the tags
 * inserted, for ASCII texts and terms / phrase words of [0-9A-Za-z_]; a text with a byte >= 0x80 is marked for the
 * CPU per item, other words are refused.  The analysis of the terms, `fields` / return_stored and the sharded and
 * coalesced paths stay with the caller.
 */
#ifndef SEARCHLITE_GPU_H
#define SEARCHLITE_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLG_ABI_VERSION 3u  /* 3: slg_tuning grew (updatable, uniform_plans, score_waves_per_simd); index updates (slg_index_update_deleted / _add_segment /
                               _remove_segment / _generation); request coalescer; slg_batch_device_candidates.
                               2: pool_cap_mb, uniform_kernel, uniform_sigma_x100, inline_cuts; shard groups; slg_batch_prepare_plans */
#define SLG_NO_TERM 0xFFFFFFFFu      /* term absent from a segment (api/reader.rs:2989) */
#define SLG_NO_VECTOR 0xFFFFFFFFu    /* vectors/mod.rs:65-67 (u32::MAX offset) */
#define SLG_MAX_QUERY_TERMS 32u      /* scored terms per query per segment */
#define SLG_MAX_K 20001u             /* k = min(max(candidate_size, limit), 20000) + 1 (api/reader.rs:2615-2619) */
#define SLG_MAX_RERANK_K 1024u       /* largest k_out of slg_rerank_*: the reference's own cap on a vector
                                        clause's k (MAX_VECTOR_K, api/reader.rs:136) */
#define SLG_MAX_VECTOR_CLAUSES 8u    /* MAX_VECTOR_CLAUSES, api/reader.rs:134 */
#define SLG_MAX_VECTOR_CANDIDATES 10000u  /* MAX_VECTOR_CANDIDATE_SIZE, api/reader.rs:138 */
#define SLG_BLOCK_SIZE 128u          /* index/postings.rs:11 DEFAULT_BLOCK_SIZE */

/* return codes (searchlite-ffi/src/lib.rs returns NULL / -1..-5 / 0) */
enum {
  SLG_OK = 0,
  SLG_ERR_INVALID = -1,     /* bad argument / malformed arrays */
  SLG_ERR_DEVICE = -2,      /* HIP runtime error, no gfx950 device */
  SLG_ERR_OOM = -3,         /* host or device allocation failed */
  SLG_ERR_UNSUPPORTED = -4, /* request shape outside the eligibility predicate */
  SLG_ERR_INTERNAL = -5
};

/* api/types.rs:6-13 ExecutionStrategy.  All three return the exhaustive-exact top-k
 * (the reference's own parity standard: tests/pruning.rs:44-104 Bm25 == Wand == Bmw).
 * Scores are ordered by f32 total_cmp (-0.0 below +0.0), as RankedDoc::cmp does
 * (query/wand.rs:30-37). */
enum { SLG_STRATEGY_BM25 = 0, SLG_STRATEGY_WAND = 1, SLG_STRATEGY_BMW = 2 };

/* index/manifest.rs VectorMetric */
enum { SLG_METRIC_COSINE = 0, SLG_METRIC_L2 = 1 };

typedef struct slg_index slg_index; /* device-resident index (all segments of one shard) */
typedef struct slg_batch slg_batch; /* one prepared query batch */

/*
 * One searchlite segment, in exactly the decoded form `search_segment` hands the scorer
 * (api/reader.rs:2985-3000): per-term posting lists (PostingsReader, index/postings.rs:133-139)
 * as a CSR over terms, per-field dense doc-length vectors (field_lengths_for,
 * api/reader.rs:3604-3621), avg field length (index/segment.rs:848), live_docs, and the
 * index-wide BM25 parameters (IndexOptions, api/types.rs:16-26).
 * All host arrays are borrowed for the duration of slg_index_create only.
 */
typedef struct {
  uint32_t n_docs;               /* seg.meta.doc_count */
  uint32_t n_terms;              /* V: number of "field:term" keys */
  const uint64_t *term_offsets;  /* [V+1] postings CSR; df(t) = off[t+1]-off[t] */
  const uint32_t *doc_ids;       /* [P] strictly increasing within a term */
  const uint32_t *tfs;           /* [P] term_freq */
  const uint16_t *term_field;    /* [V] field id of each term, NULL => field 0 */
  uint32_t n_fields;
  const float *const *field_doc_len; /* [n_fields] each f32[n_docs] (0 => missing) or NULL */
  const float *field_avgdl;          /* [n_fields] seg.avg_field_length(field) */
  float docs;                        /* seg.live_docs() as f32 */
  float k1, b;                       /* options.bm25_k1 / bm25_b */
  const uint8_t *deleted;            /* bitmap, bit (d&7) of byte d>>3; NULL => none */
  /* optional vector field for slg_rerank_batch (vectors/mod.rs:10-17 VectorStore) */
  uint32_t vec_dim;                  /* 0 => no vectors */
  int32_t vec_metric;                /* SLG_METRIC_* */
  const uint32_t *vec_offsets;       /* [n_docs] row index or SLG_NO_VECTOR */
  const float *vec_values;           /* [vec_rows * vec_dim] row-major (cosine: pre-normalized,
                                        index/segment.rs:508-510) */
  uint32_t vec_rows;
} slg_segment_desc;

/* query/wand.rs:45-50 QueryStats, per query, with brute_force's accounting (wand.rs:472,500-503)
 * applied to the work the device did:
 *   scored_docs = candidates_examined = distinct docs that got a score.  SLG_STRATEGY_BM25: every
 *     doc holding a query term (tombstoned docs included, and docs a doc filter or minimum_should_match
 *     refuses: accept() runs at top-k insertion) — the count brute_force reports.  SLG_STRATEGY_WAND / _BMW: the same when the batch runs unclassified
 *     (slg_tuning.pruning: the default for queries of <= 8 terms unless block skipping pays); with the
 *     MaxScore classification kept, docs of the ESSENTIAL lists only (a doc found in non-essential
 *     lists alone is never scored);
 *   postings_advanced = postings of the query's lists minus those block skipping never loaded.
 * Under Wand / Bmw these are NOT the reference's wand_loop counters (wand.rs:826-835, 883-891 count
 * the pivot sequence of its cursors, which the device does not walk): a caller that derives
 * total_hits_estimate from them gets a different (larger, closer to the true match count) estimate
 * than searchlite's CPU path, whose own figure under Wand / Bmw already depends on what pruning
 * skipped.  Only the Bm25 numbers are comparable across the two paths. */
typedef struct {
  uint64_t scored_docs;
  uint64_t candidates_examined;
  uint64_t postings_advanced;
} slg_stats;

/* One query = the folded term list search_segment builds (api/reader.rs:2971-3000):
 * distinct terms, weight = summed boost, term i is ScorePlan leaf i. */
typedef struct {
  uint32_t n_terms;
  const uint32_t *term_ids; /* [n_terms * n_segs]: entry [i*n_segs + s] = id of term i in
                               segment s's dictionary, or SLG_NO_TERM */
  const float *weights;     /* [n_terms] */
} slg_query;

/* ---- lifecycle ------------------------------------------------------------------- */

uint32_t slg_abi_version(void);

/* Thread-local description of the last failure on this thread ("" if none), and its code
 * (SLG_OK if none): functions that return a handle report the reason here. */
const char *slg_last_error(void);
int slg_last_error_code(void);

/* Number of visible HIP devices, or negative error. */
int slg_device_count(void);

/*
 * Stage segments into HBM on `device` and precompute per-posting BM25 impacts
 * (query/bm25.rs:1-6 + query/wand.rs:269-286 with weight factored out).  Returns NULL on
 * error (see slg_last_error).  The handle may be shared by host threads: batch planning
 * takes no lock, launches are serialized, waits happen outside the lock.
 */
slg_index *slg_index_create(const slg_segment_desc *segs, uint32_t n_segs, int device);
/* Destroys the index.  Batches prepared on it that are still alive are detached first: their
 * device buffers are freed, every later call on them fails with SLG_ERR_INVALID, and
 * slg_batch_destroy on them stays valid (so either destruction order is safe). */
void slg_index_destroy(slg_index *index);

/*
 * Tuning knobs of the batch planner, fixed per index at creation (they never change results,
 * only how the work is cut).  slg_tuning_default() fills the defaults and then applies the
 * SLG_* environment overrides named below: it is the ONLY place the library reads the
 * environment.  slg_index_create(segs, n, dev) == slg_index_create_tuned(segs, n, dev, NULL),
 * NULL meaning slg_tuning_default().
 */
typedef struct {
  uint32_t struct_size;          /* sizeof(slg_tuning) */
  int32_t validate;              /* SLG_VALIDATE (1): check every posting at staging; 0: only the
                                    last doc id of each list (ids < n_docs is always enforced) */
  int32_t champions;             /* !SLG_NO_CHAMPIONS (1): per-term champion table = threshold seed */
  int32_t allow_any_arch;        /* SLG_ALLOW_ANY_ARCH (0) */
  int32_t pruning;               /* SLG_MAXSCORE (-1): MaxScore classification, strategies Wand/Bmw.  -1 auto =
                                    batches with a query of >= 5 terms are classified and keep it if block
                                    skipping is expected to leave >= 15 % of the postings unread (else the
                                    batch runs unclassified on the few-term kernel); 0 off; 1 on */
  uint32_t uniform_max_terms;    /* SLG_UNIFORM_MAX_TERMS (8): lists the few-term kernel takes, <= 8 */
  uint32_t uniform_round_target; /* SLG_UNIFORM_ROUND_TARGET (0 = auto): postings per round */
  uint32_t multi_round_target;   /* SLG_MULTI_ROUND_TARGET (448) */
  uint32_t probe_target;         /* SLG_PROBE_TARGET (2048): postings per round incl. probed lists */
  uint32_t rounds_per_slice;     /* SLG_ROUNDS_PER_SLICE (0 = auto) */
  uint32_t max_rounds_per_slice; /* SLG_MAX_ROUNDS_PER_SLICE (0 = auto: 8 few-term kernel, 16 many-term) */
  uint32_t slices_per_subquery;  /* SLG_SLICES_PER_SUBQUERY (16) */
  int32_t cand_mode;             /* (1, reserved): k > 256 always runs via candidates + select; any other
                                    value is SLG_ERR_UNSUPPORTED (the register top-k kernels stop at k = 256) */
  int32_t slice_order;           /* !SLG_NO_SLICE_ORDER (1): longest slices launch first */
  int32_t block_max;             /* !SLG_NO_BLOCK_MAX (1): block skipping — 64-posting blocks of
                                    pruning-classified lists whose doc range holds no candidate doc
                                    are not loaded (query/wand.rs:205-265) */
  uint32_t pool_cap_mb;          /* SLG_POOL_CAP_MB (0 = auto): MiB of freed batch work buffers the
                                    index keeps for reuse; auto = a quarter of the HBM free after
                                    staging, within [1 GiB, 24 GiB].  The pool is drained whenever a
                                    device allocation of the library fails (slg_index_trim_pool) */
  uint32_t uniform_kernel;       /* SLG_UNIFORM_KERNEL (4): form of the few-term scoring kernel; 4 (blocked
                                    layout, <= 8 lists) is the only one.  2 and 3, earlier forms, were
                                    removed: SLG_ERR_UNSUPPORTED; any other value SLG_ERR_INVALID */
  uint32_t uniform_sigma_x100;   /* SLG_UNIFORM_SIGMA (0 = 320): the few-term planner keeps a round's
                                    expected lanes + this many hundredths of a sigma under 64.3 */
  int32_t inline_cuts;           /* SLG_INLINE_CUTS (-1 = auto: on): the blocked few-term kernel cuts the lists at
                                    its slice's round boundaries itself instead of reading cut points that
                                    partition_rounds_kernel wrote for the whole batch; 0 off; 1 on */
  int32_t updatable;             /* !SLG_NOT_UPDATABLE (1): keep term frequencies and doc lengths resident
                                    (4 B per posting + 4 B per doc and field) so that slg_index_update_deleted
                                    can re-derive a segment's impacts on the device when live_docs changes;
                                    0: that call fails with SLG_ERR_UNSUPPORTED (add / remove segment still work) */
  int32_t uniform_plans;         /* !SLG_NO_UNIFORM_PLANS (1): batches with flat score plans (Sum / DisMax over leaves
                                    of one or more terms) and <= uniform_max_terms lists per sub-query run on the
                                    few-term kernel's plan instantiation; 0: on the many-term kernel, as two-level
                                    plans do (A/B timing) */
  uint32_t score_waves_per_simd; /* reserved, must be 0: the few-term kernel launches one wave per slice.  Persistent
                                    scoring waves, which a non-zero value once selected, were removed (slower on
                                    MI355X): SLG_ERR_UNSUPPORTED */
} slg_tuning;
void slg_tuning_default(slg_tuning *out);
slg_index *slg_index_create_tuned(const slg_segment_desc *segs, uint32_t n_segs, int device,
                                  const slg_tuning *tuning_or_null);
int slg_index_get_tuning(const slg_index *index, slg_tuning *out);

/* Gives the freed batch work buffers the index keeps for reuse back to the runtime (the library
 * does the same by itself when one of its device allocations runs out of memory).  Call it before
 * another consumer of the device (a second index, RCCL, the application) needs the memory. */
int slg_index_trim_pool(slg_index *index, uint64_t *freed_bytes_or_null);

/* Bytes of HBM held by the index; total postings; segments. */
int slg_index_info(const slg_index *index, uint32_t *n_segs, uint64_t *n_postings,
                   uint64_t *device_bytes);

/* The champion table of segment `seg` in the index's current state, as the query planner reads it (its host copy
 * of what the staging kernel wrote; nothing is launched): out[n_terms * 68], one row of 68 floats per term, built
 * over the term's live postings.  Entries 0..63: exact-rank lower bounds, descending: at least r + 1 live postings
 * have an impact (weight 1) >= row[r]; row[0] is the list's exact maximum, the upper bound MaxScore classifies by;
 * 0 where the list is shorter.  Entries 64..67: lower bounds of the impacts at ranks 128, 256, 512 and 1024 (0
 * where no bound is known).  A segment without postings has an all-zero table.  SLG_ERR_INVALID for a NULL index,
 * a NULL out or an unknown segment; SLG_ERR_UNSUPPORTED when the index was created with slg_tuning.champions = 0. */
int slg_index_fetch_champions(const slg_index *index, uint32_t seg, float *out);

/* ---- index updates (the reference's commit: api/writer.rs:106-240) -------------------------------
 * searchlite opens a fresh IndexReader per request (searchlite-http/src/lib.rs:640-643 ->
 * index/mod.rs:98-100 -> api/reader.rs:1887-1913), so a staged index must outlive readers and follow
 * the manifest: a commit merges new tombstones into segments' deleted_docs (api/writer.rs:150-158:
 * the set only grows), appends at most one new segment (:160-192, at the END of manifest.segments, so
 * existing segment ordinals keep their meaning) and compaction replaces segments (index/mod.rs:102+).
 *
 * The index is a sequence of immutable states.  Every call below builds the next state (unchanged
 * segments are shared, not copied), publishes it atomically and bumps the generation.  A batch is
 * bound to the state that was current when it was PREPARED: batches prepared or in flight during an
 * update run to completion against their own state — same segments, same tombstones, same filters —
 * and the device memory of a retired state is released when its last batch is destroyed.  Updates are
 * serialised among themselves and never wait for running batches.
 *
 * The caller builds q_term_ids rows for the segment count it knows: it must not race
 * slg_index_add_segment / _remove_segment with building query arrays for the same index (the Rust
 * shim holds these calls under the index's write lock; slg_index_generation tells a reader whether
 * the staged index still matches its manifest snapshot). */

/* New tombstones for segment `seg`: `deleted` is the segment's COMPLETE bitmap (bit d&7 of byte d>>3;
 * a superset of the previous one — the reference never resurrects a doc), `live_docs` =
 * seg.live_docs() = doc_count - |deleted| (index/segment.rs:1365-1370).  live_docs is the `docs` of
 * every ScoredTerm (api/reader.rs:2985), so every idf — and with it every posting's impact, every
 * champion bound and threshold seed — changes: they are re-derived on the device from the resident
 * term frequencies and doc lengths by the same kernels as at creation, i.e. bit-identical to a fresh
 * slg_index_create on the updated descriptor.  Registered filters follow (their reject bitmaps of
 * this segment take the new tombstones).  Needs slg_tuning.updatable. */
int slg_index_update_deleted(slg_index *index, uint32_t seg, const uint8_t *deleted, float live_docs);
/* Stage one more segment; it takes the next ordinal (returned, >= 0; negative error code otherwise).
 * Filters registered before the call have no bitmap for it: a batch that names one of them fails with
 * SLG_ERR_INVALID until the filter is removed and registered again.  Extra vector fields
 * (slg_index_add_vector_field) hold no vectors for the new segment. */
int slg_index_add_segment(slg_index *index, const slg_segment_desc *seg);
/* Drop segment `seg` (compaction, index/mod.rs:102+); the ordinals above it move down by one. */
int slg_index_remove_segment(slg_index *index, uint32_t seg);
/* The HIP device the index lives on (>= 0), or a negative error code. */
int slg_index_device(const slg_index *index);
/* Number of updates applied since creation (0 for a fresh index). */
uint64_t slg_index_generation(const slg_index *index);

/* Use an external HIP stream (hipStream_t) for all work of this index, e.g. the current
 * PyTorch stream so RCCL collectives order after the kernels.  NULL is a valid handle (the
 * HIP null stream, which is what PyTorch's default stream is); SLG_OWN_STREAM restores the
 * index's own non-blocking stream. */
#define SLG_OWN_STREAM ((void *)(intptr_t)-1)
int slg_index_set_stream(slg_index *index, void *hip_stream);

/* ---- doc filters ----------------------------------------------------------
 * The reference's accept() is `!deleted && matcher && filter && cursor`
 * (api/reader.rs:3009-3036); for a pure disjunction the matcher is implied and a filter
 * (query/filters.rs: keyword equality / numeric range on fast fields) reduces to a doc bitmap.
 * A filter is registered once per index and referenced by id from any number of queries.
 * All return a filter id >= 0, or a negative error code. */

/* seg_bitmaps[s]: bit d of byte d/8 set = doc d of segment s passes; NULL = all pass. */
int slg_index_add_filter(slg_index *index, const uint8_t *const *seg_bitmaps);
/* Pre-pass on the device: doc d passes iff lo <= column[d] <= hi (one fast-field column per
 * segment, n_docs values; a NaN never passes). */
int slg_index_add_filter_range_i64(slg_index *index, const int64_t *const *seg_columns, int64_t lo,
                                   int64_t hi);
int slg_index_add_filter_range_f64(slg_index *index, const double *const *seg_columns, double lo,
                                   double hi);
/* A filter from posting lists that are already on the device: the docs that hold NONE of the given terms
 * (pass_if_absent != 0: the query-string matcher's not-terms, api/reader.rs:1499-1503 — a doc in any
 * not-term group never matches) or at least one of them (pass_if_absent == 0).  term_ids: n_terms rows of
 * one id per segment (SLG_NO_TERM: the segment does not have the term), as in slg_query.  and_bitmaps_or_null:
 * pass bitmaps as in slg_index_add_filter, AND-ed with the above (the request's own filter), or NULL.
 * Returns the filter id (>= 0) or an error code; use it like any other filter id. */
int slg_index_add_filter_terms(slg_index *index, const uint32_t *term_ids, uint32_t n_terms, int pass_if_absent,
                               const uint8_t *const *and_bitmaps_or_null);
/* Unregisters the filter.  Batches already prepared with it keep their bitmaps (they belong to the
 * batch's index state) and may still run; the id may be handed out again by a later add. */
int slg_index_remove_filter(slg_index *index, int filter_id);

/* ---- filter trees built on the device (query/filters.rs:84-149; index/fastfields.rs:490-640) ----
 * A filter tree (api/types.rs: KeywordEq, KeywordIn, I64Range, F64Range, And, Or, Not) over the columns
 * registered with slg_index_add_agg_field_* is evaluated on the device, doc by doc, into the reject bitmap every
 * batch kind reads.  A tree is a POSTFIX program: a leaf pushes one value, AND / OR replace the `arity` values on
 * top of the stack by one, NOT replaces the top; the program ends with exactly one value.
 *   KEYWORD_IN  field: a keyword column.  Passes iff ANY ordinal of the doc is in ords[ord_begin .. ord_begin +
 *               n_ords_in) of the tree (repeats allowed; an empty set passes nothing).  The caller resolves
 *               KeywordEq / KeywordIn strings to ordinals with the reference's case_insensitive_equals: several
 *               dictionary keys may fold to one value.  An ordinal >= the field's n_ords: SLG_ERR_INVALID.
 *   RANGE_F64   field: a numeric column.  Passes iff any value v of the doc has lo_f <= v && v <= hi_f in IEEE
 *               f64: a NaN value never passes, infinite bounds are allowed, a NaN bound is SLG_ERR_INVALID.  A
 *               column that holds non-finite values is accepted (the comparison is well defined).
 *   RANGE_I64   field: a numeric column registered with slg_index_add_agg_field_i64 (on an _f64 column:
 *               SLG_ERR_INVALID).  The column holds `v as f64`: one whose finite minimum or maximum lies outside
 *               +-2^53 is refused with SLG_ERR_UNSUPPORTED (those values were rounded at registration);
 *               otherwise lo_i / hi_i are clamped into +-2^53 and compared in f64, which is exact (a lo_i above
 *               2^53 or a hi_i below -2^53 passes nothing: it is compared as the infinity, not as the clamped value,
 *               which a stored +-2^53 would equal).
 *   FILTER_ID   filter_id: a registered filter of any kind.  Passes iff its reject bit is clear.  That bitmap
 *               already holds the tombstones, so NOT over this leaf passes deleted docs inside the tree; the
 *               final bitmap ORs the tombstones in again, so the result is right all the same.  This leaf is how
 *               not-term filters and any host-made bitmap compose with the rest (Nested nodes are evaluated on the
 *               device too: slg_index_add_nested_filter_trees below).
 *   AND / OR    arity children (0 and up): AND of none is true (passes_filters_at on an empty list), OR of none
 *               is false.  NOT: exactly one child.
 * A doc without a value fails every leaf over that column (NOT of the leaf then passes it); so does every doc of
 * a segment registered with seg_offsets[s] == NULL.  Final bitmap of every segment: reject = deleted | ~tree;
 * bits past n_docs are set. */
enum { SLG_FILTER_KEYWORD_IN = 0, SLG_FILTER_RANGE_F64 = 1, SLG_FILTER_RANGE_I64 = 2, SLG_FILTER_ID = 3,
       SLG_FILTER_AND = 4, SLG_FILTER_OR = 5, SLG_FILTER_NOT = 6 };
#define SLG_MAX_FILTER_NODES 64u   /* nodes of one tree */
#define SLG_MAX_FILTER_DEPTH 16u   /* deepest evaluation stack */
#define SLG_MAX_FILTER_TREES 64u   /* trees of one call */
typedef struct slg_filter_node {
  int32_t kind;        /* SLG_FILTER_* */
  int32_t field;       /* agg field id (KEYWORD_IN, RANGE_*) */
  int32_t filter_id;   /* FILTER_ID */
  uint32_t arity;      /* AND / OR */
  double lo_f, hi_f;   /* RANGE_F64 */
  int64_t lo_i, hi_i;  /* RANGE_I64 */
  uint32_t ord_begin, n_ords_in;  /* KEYWORD_IN: a range of the tree's ords */
} slg_filter_node;
typedef struct slg_filter_tree {
  uint32_t n_nodes;
  const slg_filter_node *nodes;
  uint32_t n_ords;
  const uint32_t *ords;
} slg_filter_tree;
/* Registers n_trees filters in ONE update of the index's state (a retired state costs a device synchronise: n
 * filters must not cost n updates); out_ids[t] is the filter id of trees[t], handed out as by slg_index_add_filter
 * (lowest free ids).  All or nothing: on an error no id is handed out and the index is as it was.  Afterwards the
 * filters are ordinary filters (slg_index_remove_filter, slg_index_update_deleted, slg_index_add_segment and
 * slg_index_remove_segment treat them like any other).  Errors, in this order: SLG_ERR_INVALID before the index
 * is looked at (NULL arrays; n_trees == 0 or n_nodes == 0; an unknown kind; a program that underflows the stack or
 * does not end with exactly one value; an arity larger than the stack; a NaN bound; ord_begin + n_ords_in >
 * n_ords), then SLG_ERR_UNSUPPORTED (more than SLG_MAX_FILTER_NODES nodes, a stack deeper than
 * SLG_MAX_FILTER_DEPTH, more than SLG_MAX_FILTER_TREES trees), then against the index SLG_ERR_INVALID (an unknown
 * field or filter id; a field or filter without data for every segment; the wrong column kind; an ordinal out of
 * range), then SLG_ERR_UNSUPPORTED for the 2^53 rule.  Returns 0 or an error code. */
int slg_index_add_filter_trees(slg_index *index, const slg_filter_tree *trees, uint32_t n_trees, int32_t *out_ids);
/* ---- nested filters on the device (query/filters.rs:13-188; index/fastfields.rs:802-907) ----
 * A Nested{path, filter} node (api/types.rs) matches a doc iff SOME object of the array of objects at `path`
 * passes `filter` as a whole: its leaves read the values of that ONE object.  The device evaluates such trees over
 * nested paths and nested value columns registered here, the arrays the fast-field file holds for them.
 *
 * A nested PATH (the reference's _nested_count:<path> and _nested_parent:<path> columns), per segment:
 *   seg_counts[s][n_docs]            objects per doc; seg_counts == NULL or seg_counts[s] == NULL: no doc has one
 *   seg_parent_offsets[s][n_docs+1]  CSR into seg_parents[s]: entry j of a doc is the index, within the same doc, of
 *   seg_parents[s]                   the parent path's object that child object j belongs to; 0xFFFFFFFF: none.  A
 *                                    list shorter than the doc's count leaves the rest unbound; NULL offsets (or a
 *                                    NULL array of them): nothing binds.
 * parent_path_id: the id of the path one level up (e.g. `comment` for `comment.reply`), or -1.  It is what a
 * NESTED node inside an object scope is checked against; at the doc level no parent test is made, whatever the
 * path.  The host builds the docs' first objects (the prefix sum of the counts) and the object -> doc table; a
 * segment with more than 2^32 - 1 objects is SLG_ERR_UNSUPPORTED.  Returns the path id (>= 0; ids are never
 * reused) or an error code.  Lifecycle as aggregation fields: slg_index_update_deleted keeps the tables,
 * slg_index_remove_segment drops that segment's, slg_index_add_segment gives the new segment none (a tree naming
 * the path is then SLG_ERR_INVALID, "nested path N has no tables for segment S", until it is registered again);
 * batches prepared earlier keep their state.  Removing a path removes the nested fields registered under it; a
 * path registered with it as parent stays, usable at the doc level. */
int slg_index_add_nested_path(slg_index *index, int parent_path_id, const uint32_t *const *seg_counts,
                              const uint32_t *const *seg_parent_offsets, const uint32_t *const *seg_parents);
int slg_index_remove_nested_path(slg_index *index, int path_id);
/* A nested VALUE column `<path>.<field>` (the reference's I64Nested / F64Nested / StrNested columns), per segment:
 *   seg_doc_offsets[s][n_docs+1]     the doc's objects in seg_object_offsets[s]; NULL: the segment has no value
 *   seg_object_offsets[s][objects+1] the object's values in seg_values[s]
 * A doc may hold FEWER objects here than its path counts (the writer pads only up to the last object that had a
 * value): an object beyond them has no value.  _i64 columns stay int64 on the device and are compared as
 * integers: the +-2^53 rule of the doc-level RANGE_I64 does not apply to them.  _ord: ordinals into ONE caller-side
 * dictionary of n_ords keys, as slg_index_add_agg_field_ord (an ordinal >= n_ords: SLG_ERR_INVALID).  Offsets that
 * decrease, or a NULL array behind a non-empty range: SLG_ERR_INVALID.  Returns the nested field id (>= 0; ids are
 * never reused) or an error code; lifecycle as the paths. */
int slg_index_add_nested_field_f64(slg_index *index, int path_id, const uint32_t *const *seg_doc_offsets,
                                   const uint32_t *const *seg_object_offsets, const double *const *seg_values);
int slg_index_add_nested_field_i64(slg_index *index, int path_id, const uint32_t *const *seg_doc_offsets,
                                   const uint32_t *const *seg_object_offsets, const int64_t *const *seg_values);
int slg_index_add_nested_field_ord(slg_index *index, int path_id, const uint32_t *const *seg_doc_offsets,
                                   const uint32_t *const *seg_object_offsets, const uint32_t *const *seg_ords,
                                   uint32_t n_ords);
int slg_index_remove_nested_field(slg_index *index, int nested_field_id);
/* A nested filter tree is a list of SCOPES over one node array, children before parents; the last scope is the doc
 * level (path -1), every other one an object scope (path: a nested path id).  A scope's nodes
 * nodes[node_begin .. node_begin + n_nodes) are a postfix program as above.
 *   doc level     the seven kinds above with their meaning (the 2^53 rule included), and
 *                 NESTED  field: the index of an earlier scope of the tree.  Passes iff SOME object of that scope's
 *                         path in the doc passes that scope's program; a doc without objects never passes (NOT of
 *                         the leaf passes it).  No parent test is made, even for a path that has a parent.
 *   object scope  KEYWORD_IN / RANGE_F64 / RANGE_I64  field: a NESTED FIELD id.  ANY value of the scope's object
 *                         may satisfy the leaf; an object without a value fails it.  The kind must fit the column
 *                         (SLG_ERR_INVALID otherwise); a field registered under ANOTHER path passes nothing (the
 *                         reference finds no such column).  RANGE_I64 compares int64 with int64.
 *                 AND / OR / NOT as above.
 *                 NESTED  field: an earlier scope whose path's registered parent is THIS scope's path
 *                         (SLG_ERR_INVALID otherwise).  Passes iff some object of that path in the doc passes its
 *                         scope AND its entry of the parent list names this scope's object.
 *                 FILTER_ID is SLG_ERR_INVALID here.
 * Every scope but the last is named by exactly one NESTED node.  The Nested children of ONE And that share a path
 * must hold for ONE object (passes_filters_at): the caller folds them into one scope whose program ANDs them; under
 * Or and Not, and for a lone Nested, every node has a scope of its own. */
#define SLG_FILTER_NESTED 7
#define SLG_MAX_NESTED_SCOPES 16u  /* scopes of one tree, the doc level included */
#define SLG_MAX_NESTED_DEPTH 4u    /* object scopes below one another */
typedef struct slg_nested_scope {
  int32_t path;         /* nested path id; -1: the doc level (the last scope, and only it) */
  uint32_t node_begin;  /* into the tree's nodes */
  uint32_t n_nodes;
} slg_nested_scope;
typedef struct slg_nested_filter_tree {
  uint32_t n_scopes;
  const slg_nested_scope *scopes;
  uint32_t n_nodes;
  const slg_filter_node *nodes;
  uint32_t n_ords;
  const uint32_t *ords;
} slg_nested_filter_tree;
/* Registers n_trees filters in ONE update of the index's state, all or nothing, ids as by
 * slg_index_add_filter_trees; afterwards they are ordinary filters.  The trees are evaluated level by level, the
 * deepest object scopes first: (nesting depth + 1) launches per segment, whatever the number of trees and scopes.
 * Errors, in this order: SLG_ERR_INVALID before the index is looked at (NULL arrays; n_trees, n_scopes or a
 * scope's n_nodes == 0; a scope's nodes beyond n_nodes; a last scope that is not the doc level or an earlier one
 * that is; what slg_index_add_filter_trees refuses in a program; FILTER_ID in an object scope; a NESTED node that
 * names no earlier scope; a scope named twice or never), then SLG_ERR_UNSUPPORTED (more than SLG_MAX_FILTER_NODES
 * nodes over all scopes, a scope's stack deeper than SLG_MAX_FILTER_DEPTH, more than SLG_MAX_NESTED_SCOPES scopes,
 * object scopes nested deeper than SLG_MAX_NESTED_DEPTH, more than SLG_MAX_FILTER_TREES trees), then against the
 * index SLG_ERR_INVALID (an unknown path, nested field, agg field or filter id; one without data for every segment;
 * the wrong column kind; an ordinal out of range; a NESTED node in an object scope whose path is not the child's
 * registered parent), then SLG_ERR_UNSUPPORTED for the doc level's 2^53 rule.  Returns 0 or an error code. */
int slg_index_add_nested_filter_trees(slg_index *index, const slg_nested_filter_tree *trees, uint32_t n_trees,
                                      int32_t *out_ids);
/* The PASS bits (~reject: the doc is alive and passes) of segment seg of any registered filter, whichever call
 * made it: ceil(n_docs / 8) bytes, bit d & 7 of byte d >> 3. */
int slg_index_fetch_filter(slg_index *index, int filter_id, uint32_t seg, uint8_t *out_pass);

/* ---- sort fields (query/sort.rs: `sort` on numeric fast fields) -----------------------
 * A numeric fast field registered once per index and named by id in sorted batches
 * (slg_batch_prepare_sorted).  Per segment the doc's values as CSR: seg_offsets[s][n_docs + 1] into
 * seg_values[s] (the reference's i64_values / f64_values, index/fastfields.rs:736-770: several values per
 * doc allowed); an empty range = Missing; seg_offsets[s] == NULL = every doc of segment s Missing.  The
 * library picks, on the host, the value the reference sorts by (query/sort.rs:300-345: Asc = min_by, Desc =
 * max_by under partial_cmp(..).unwrap_or(Equal) — min_by keeps the first of equal elements, max_by the
 * last; this decides NaN and -0.0 / +0.0) and keeps two device columns (an order-preserving u64 per order)
 * and a presence bitmap; host arrays are borrowed for the call only.  Lifecycle as filters:
 * slg_index_update_deleted keeps the columns, slg_index_remove_segment drops that segment's,
 * slg_index_add_segment gives the new segment none (a sorted batch that names the field then fails with
 * SLG_ERR_INVALID until it is registered again).  Return the field id (>= 0) or a negative error code;
 * ids are never handed out again, so a stale id fails instead of naming another field. */
#define SLG_MAX_SORT_PARTS 4u
#define SLG_SORT_SCORE (-1) /* the `_score` part */
enum { SLG_ORDER_ASC = 0, SLG_ORDER_DESC = 1 };
int slg_index_add_sort_field_i64(slg_index *index, const uint32_t *const *seg_offsets,
                                 const int64_t *const *seg_values);
int slg_index_add_sort_field_f64(slg_index *index, const uint32_t *const *seg_offsets,
                                 const double *const *seg_values);
/* Batches already prepared with the field keep its columns (they belong to the batch's index state). */
int slg_index_remove_sort_field(slg_index *index, int sort_field_id);

/* ---- one-shot search (what a searchlite `gpu` shim calls) -------------------------- */

/*
 * Replaces, for a batch of eligible queries, the per-segment scorer call plus the
 * cross-segment sort: for every query, top-k by (score desc [f32 total_cmp],
 * segment_ord asc, doc_id asc) over all segments of the index.
 * Outputs are caller-owned host arrays of nq*k (out_count: nq); row q holds
 * out_count[q] <= k hits.  Blocks until the results are in the output arrays.
 */
int slg_search_batch(slg_index *index, const slg_query *queries, uint32_t nq, uint32_t k,
                     int strategy, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                     uint32_t *out_count, slg_stats *stats_or_null);

/* Same with a doc filter per query (q_filter[q] = filter id, < 0 none; NULL = none at all). */
int slg_search_batch_filtered(slg_index *index, const slg_query *queries, uint32_t nq,
                              const int32_t *q_filter, uint32_t k, int strategy, uint32_t *out_doc,
                              uint32_t *out_seg, float *out_score, uint32_t *out_count,
                              slg_stats *stats_or_null);

/* ---- prepared batches (device-resident inputs; used for steady-state serving) ------ */

/*
 * Queries in CSR form: q_offsets[nq+1] indexes q_weights and the rows of q_term_ids
 * ([total_terms * n_segs], same layout as slg_query.term_ids).  Plans the batch on the
 * host, uploads the descriptors and allocates all device work buffers.
 */
slg_batch *slg_batch_prepare(slg_index *index, uint32_t nq, const uint32_t *q_offsets,
                             const uint32_t *q_term_ids, const float *q_weights, uint32_t k,
                             int strategy);
/* Same, with a doc filter per query: q_filter[q] = filter id, or < 0 for none (q_filter may be
 * NULL).  Filtered queries get no threshold seed (the filter may reject the champions). */
slg_batch *slg_batch_prepare_filtered(slg_index *index, uint32_t nq, const uint32_t *q_offsets,
                                      const uint32_t *q_term_ids, const float *q_weights,
                                      const int32_t *q_filter, uint32_t k, int strategy);
/* Same with a score plan per query (query/planner.rs:113-153).  q_tie[q] must lie in
 * [0, 1] (validate_tie_breaker, query/planner.rs:850-856) and leaves must be < 2^31.  The reference adds
 * every scored term's contribution to a ScorePlan leaf (wand.rs:488-497 `buf[term.leaf] +=`) and
 * combines the leaves: a multi-field query string maps all fields of a word to one leaf and sums
 * the leaves; multi_match best_fields / dis_max take DisMax over the leaves.
 *   q_leaf[i]   leaf of query term i (same indexing as q_weights); NULL: term i of a query is
 *               leaf i (the plain disjunction)
 *   q_plan[q]   SLG_PLAN_SUM or SLG_PLAN_DISMAX over the leaves; NULL: SUM
 *   q_tie[q]    DisMax tie breaker (max + tie * (sum - max)); NULL: 0
 *   q_nleaves[q] leaves of the plan (>= max leaf + 1; leaves without a term count as 0.0 in a
 *               DisMax); NULL: max leaf + 1
 * Results are bit-identical to the reference's exhaustive scorer (per-leaf sums in term order,
 * leaves combined in leaf order). */
#define SLG_PLAN_SUM 0
#define SLG_PLAN_DISMAX 1
slg_batch *slg_batch_prepare_plan(slg_index *index, uint32_t nq, const uint32_t *q_offsets,
                                  const uint32_t *q_term_ids, const float *q_weights,
                                  const uint32_t *q_leaf, const int32_t *q_plan, const float *q_tie,
                                  const uint32_t *q_nleaves, const int32_t *q_filter, uint32_t k,
                                  int strategy);

/* Two-level score plans.  ScoreExpr::evaluate is recursive (query/planner.rs:122-153) and real
 * requests build two-level trees: `dis_max{queries}` = a DisMax of sub-scorers
 * (planner.rs:470-487), `bool{should:[multi_match ...]}` = a Sum of DisMax groups
 * (planner.rs:670-690).  Here the ROOT (q_plan / q_tie) combines GROUPS, a group (group_plan /
 * group_tie) combines LEAVES, a leaf sums the scored terms that name it (wand.rs:488-497).
 * Leaves are numbered in the plan's traversal order, so a group's leaves are consecutive:
 * leaf_group is non-decreasing within a query and names every group 0 .. n_groups-1.  A leaf that
 * hangs off the root directly is a SLG_PLAN_SUM group of one leaf (Sum of one child is the child,
 * bit for bit).  With leaf_group == NULL this is slg_batch_prepare_plan.  Every DisMax counts all
 * of its children, the ones without a posting for a doc as 0.0, as the reference does. */
typedef struct {
  const uint32_t *q_leaf;           /* [total terms] leaf of every query term; NULL: term i = leaf i */
  const int32_t *q_plan;            /* [nq] root: SLG_PLAN_SUM | SLG_PLAN_DISMAX; NULL: Sum */
  const float *q_tie;               /* [nq] root tie breaker in [0, 1]; NULL: 0 */
  const uint32_t *q_nleaves;        /* [nq] leaves of the plan; NULL: 1 + the largest leaf named */
  const uint32_t *q_leaf_offsets;   /* [nq + 1] into leaf_group (two-level plans only) */
  const uint32_t *leaf_group;       /* group of every leaf of every query; NULL: flat plans */
  const uint32_t *q_group_offsets;  /* [nq + 1] into group_plan / group_tie */
  const int32_t *group_plan;        /* SLG_PLAN_SUM | SLG_PLAN_DISMAX per group */
  const float *group_tie;           /* tie breaker per group, in [0, 1] */
  /* Trees of any shape (ScoreExpr is recursive, query/planner.rs:113-153), up to SLG_MAX_PLAN_DEPTH levels
   * of Sum / DisMax nodes above the leaves: per query a node array in PRE-ORDER (node 0 = the root,
   * node_parent[i] < i, node_parent[0] ignored), node_kind = SLG_PLAN_SUM | SLG_PLAN_DISMAX | SLG_PLAN_LEAF,
   * node_tie in [0, 1] for DisMax nodes; the i-th LEAF node of a query in pre-order is ScorePlan leaf i
   * (q_leaf names it per query term).  Every Sum / DisMax node has at least one child.  With
   * q_node_offsets != NULL the root / group arrays above are not read (q_leaf still is).  Trees of one
   * or two levels run exactly as the forms above; deeper ones on the many-term kernel's tree mode. */
  const uint32_t *q_node_offsets;   /* [nq + 1] into node_kind / node_tie / node_parent; NULL: the forms above */
  const int32_t *node_kind;
  const float *node_tie;
  const uint32_t *node_parent;
  /* minimum_should_match of a query string (api/reader.rs:1509-1517: a doc matches if at least that many of
   * the matcher's term groups hold it; a term group = a ScorePlan leaf, i.e. one query word over its
   * fields).  [nq] or NULL; 0 and 1 = any doc of any list.  Batches with a value > 1 are accepted for flat
   * plans (one level of Sum / DisMax over the leaves) of at most 8 scored lists per segment — what the
   * few-term kernel's plan instantiation runs; other shapes: SLG_ERR_UNSUPPORTED (CPU scorer). */
  const uint32_t *q_min_match;
} slg_score_plans;
#define SLG_PLAN_LEAF 2
#define SLG_MAX_PLAN_DEPTH 4u
slg_batch *slg_batch_prepare_plans(slg_index *index, uint32_t nq, const uint32_t *q_offsets,
                                   const uint32_t *q_term_ids, const float *q_weights,
                                   const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                                   uint32_t k, int strategy);
/* Field-sorted batches (SortPlan::from_request with numeric fast fields, query/sort.rs:159-216).  One sort
 * spec for the whole batch: parts compared in order (field = a sort field id, or SLG_SORT_SCORE; order =
 * SLG_ORDER_*), a Missing value after every value in both orders, ties after all parts by segment asc, doc
 * asc (SortKey::cmp, query/sort.rs:80-123).  Rows hold the top k (k = limit + 1 <= SLG_MAX_K) by that key
 * over all segments, through slg_batch_run / _fetch / _device_results as any batch; out_score is the exact
 * score (bit-identical to the score path) when a part is `_score`, else 0.0 (ScoreMode::MatchOnly,
 * api/reader.rs:2936-2940).  Every query shape slg_batch_prepare_plans takes is accepted.  Every matched doc
 * is scored (candidates mode, no threshold seed, no MaxScore): 8 bytes of device memory per posting of the
 * batch.  More than SLG_MAX_SORT_PARTS parts or a keyword field: SLG_ERR_UNSUPPORTED (CPU scorer); an
 * unknown sort field id or one without a column for every segment: SLG_ERR_INVALID. */
typedef struct {
  uint32_t n_parts;
  int32_t field[SLG_MAX_SORT_PARTS]; /* sort field id, or SLG_SORT_SCORE */
  int32_t order[SLG_MAX_SORT_PARTS]; /* SLG_ORDER_ASC | SLG_ORDER_DESC */
} slg_sort_spec;
slg_batch *slg_batch_prepare_sorted(slg_index *index, uint32_t nq, const uint32_t *q_offsets,
                                    const uint32_t *q_term_ids, const float *q_weights,
                                    const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                                    const slg_sort_spec *sort, uint32_t k, int strategy);
/* Accepted docs per query of a sorted batch's last run (total_matches, api/reader.rs:3026-3028: docs that
 * pass tombstones, filter and minimum_should_match; in a cursor batch, of those the ones after the cursor);
 * waits for the batch.  SLG_ERR_INVALID for a batch that is neither sorted nor a cursor batch. */
int slg_batch_matched_counts(slg_batch *batch, uint64_t *out_matched);
/* One-shot form: slg_search_batch_filtered with score plans and a sort spec; out_matched ([nq]) may be NULL. */
int slg_search_batch_sorted(slg_index *index, const slg_query *queries, uint32_t nq,
                            const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                            const slg_sort_spec *sort, uint32_t k, int strategy, uint32_t *out_doc,
                            uint32_t *out_seg, float *out_score, uint32_t *out_count, uint64_t *out_matched);
/* Cursor pagination (the next page of a request: api/reader.rs:3009-3036).  The cursor key, decoded by the
 * caller from the reference's PaginationCursor / SortCursorState (api/reader.rs:613-900): the values the
 * previous page's last hit was sorted by, then its segment_ord and doc_id.  value_bits[p] of part p: an i64
 * field's value (two's complement), an f64 field's bits, or a `_score` part's f32 bits in the low 32 bits
 * (the high 32 zero); a Missing part has its missing_mask bit set (its value_bits are not read).  Parts
 * beyond the spec (score order: beyond part 0) hold zero.  has_cursor == 0: a first page (nothing else of
 * the row is read). */
typedef struct {
  uint32_t has_cursor;
  uint32_t segment_ord, doc_id;
  uint32_t missing_mask;  /* bit p: sort part p is Missing (never a `_score` part) */
  uint64_t value_bits[SLG_MAX_SORT_PARTS];
} slg_sort_cursor;
/* A batch whose rows hold, per query, the top k strictly AFTER the query's cursor in SortKey::cmp order
 * (query/sort.rs:80-123).  sort_or_null == NULL: score order (score desc by f32 total_cmp, segment asc, doc
 * asc: the score path's order, score_fast_path); value_bits[0] holds the cursor's score.  Otherwise a field
 * sort, the specs slg_batch_prepare_sorted takes, one cursor value per part.  Rows come back through
 * slg_batch_run / _fetch / _device_results; scores are bit-identical to the score path (0.0 in a field sort
 * without a `_score` part, as slg_batch_prepare_sorted).  Every matched doc is scored (candidates mode, no
 * threshold seed, no MaxScore: after a cursor the k-th eligible score lies below any champion bound).
 * slg_batch_matched_counts gives the accepted docs after the cursor (total_matches; the caller adds the
 * rows it returned before).  Checked on the host before any device work: q_cursor NULL, a Missing bit on a
 * `_score` part or beyond the spec, non-zero value_bits beyond the spec, or a `_score` value with high bits
 * set: SLG_ERR_INVALID.  A segment_ord / doc_id that names no doc is not an error (the cursor is stale).
 * slg_batch_run_sharded[_seq] and slg_batch_fetch_sharded refuse a cursor batch (SLG_ERR_UNSUPPORTED: a
 * cursor's segment_ord is index-global). */
slg_batch *slg_batch_prepare_after(slg_index *index, uint32_t nq, const uint32_t *q_offsets,
                                   const uint32_t *q_term_ids, const float *q_weights,
                                   const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                                   const slg_sort_spec *sort_or_null, const slg_sort_cursor *q_cursor,
                                   uint32_t k, int strategy);
/* Per query of a cursor batch's last run (waits): 1 when an accepted doc's key equals the cursor key (the
 * reference's saw_cursor) or the query has no cursor; 0 when the cursor doc was deleted, filtered out, scored
 * differently or names no doc — the rows are still the window after the key, and the caller decides (the
 * reference rejects such a cursor, api/reader.rs:2747-2749).  SLG_ERR_INVALID for a batch without cursors. */
int slg_batch_cursor_seen(slg_batch *batch, uint8_t *out_seen);
/* One-shot form: slg_search_batch_sorted with a cursor per query; out_matched ([nq], u64) and out_seen ([nq])
 * may be NULL. */
int slg_search_batch_after(slg_index *index, const slg_query *queries, uint32_t nq,
                           const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                           const slg_sort_spec *sort_or_null, const slg_sort_cursor *q_cursor, uint32_t k,
                           int strategy, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                           uint32_t *out_count, uint64_t *out_matched, uint8_t *out_seen);
/* Enqueue the partition / score / merge kernels on the batch's stream (asynchronous). */
int slg_batch_run(slg_batch *batch);
/* Run this batch on its own HIP stream instead of the index stream, so several prepared
 * batches can be in flight at once (their partition / merge kernels then overlap the other
 * batches' scoring).  A batch owns all its work buffers; batches never share state.
 * SLG_OWN_STREAM returns the batch to the index stream. */
int slg_batch_set_stream(slg_batch *batch, void *hip_stream);
/* Wait for everything enqueued for this batch. */
int slg_batch_sync(slg_batch *batch);
/* Copy results to host arrays (nq*k, nq); waits for completion. */
int slg_batch_fetch(slg_batch *batch, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                    uint32_t *out_count, slg_stats *stats_or_null);
/* Device pointers of the result arrays (u32[nq*k], u32[nq*k], f32[nq*k], u32[nq]) for
 * device-side consumers (RCCL all-gather of per-shard top-k, rerank). */
int slg_batch_device_results(slg_batch *batch, void **d_doc, void **d_seg, void **d_score,
                             void **d_count);
/* The four result arrays live back to back in ONE device allocation, in the order
 * doc[nq*k] | seg[nq*k] | score[nq*k] | count[nq] (4-byte elements, so (3*k+1)*nq*4 bytes):
 * a multi-GPU caller exchanges the per-shard top-k with a single all-gather of this block. */
int slg_batch_device_result_block(slg_batch *batch, void **d_block, uint64_t *n_bytes);
/* Planning facts: total postings the batch scores, number of work slices, and the
 * algorithmic byte count 12*postings + 8*k*nq. */
int slg_batch_info(const slg_batch *batch, uint64_t *n_postings, uint32_t *n_slices,
                   uint64_t *algorithmic_bytes);
/* Block skipping (query/wand.rs:205-265), last run of the batch: postings of the batch's
 * pruning-classified (non-essential) lists, and how many of them were never loaded — their
 * 64-posting block, or their whole round, held no candidate doc.  Blocks are tested only in lists
 * much denser than the query's essential lists.  Both 0 when the batch has no classified list or
 * slg_tuning.block_max is off.  Waits for the batch. */
int slg_batch_skip_counts(slg_batch *batch, uint64_t *probed_postings, uint64_t *skipped_postings);
void slg_batch_destroy(slg_batch *batch);

/* ---- aggregations (query/aggs/mod.rs: `aggs` with terms, histogram, range, stats, cardinality, percentiles
 * and percentile_ranks) -----------------------------------------------------------------------------
 * A request with `aggs` makes the reference visit every matched doc (a collector sets the WAND threshold to
 * -inf, query/wand.rs:725-729) and upsert a hash map per aggregation and doc (aggs/mod.rs:894-930,
 * 1166-1204).  On the device an aggregation batch is planned like a sorted batch — every matched doc is a
 * candidate, once, with its exact score — and one more kernel walks the candidates and fills dense bucket
 * tables.  The aggregated set of a query is exactly the docs slg_batch_matched_counts counts: those that
 * pass tombstones, the doc filter and minimum_should_match (api/reader.rs:3009-3036), over all segments,
 * whatever k is.  The rows of an aggregation batch are bit-identical to the same batch without aggregations.
 *
 * Columns are registered once per index and named by id, with the lifecycle and id policy of sort fields:
 * per segment a CSR (seg_offsets[s][n_docs + 1] into seg_values[s]; an empty range = the doc has no value;
 * seg_offsets[s] == NULL = no doc of segment s has one); slg_index_update_deleted keeps the columns,
 * slg_index_remove_segment drops that segment's, slg_index_add_segment gives the new segment none (a batch
 * that names the field then fails with SLG_ERR_INVALID until it is registered again); ids are never handed
 * out again.  Numeric columns hold f64 (an i64 field arrives as `v as f64`, index/fastfields.rs:772-800, the
 * conversion done here on the host); registration records, per segment, the finite minimum and maximum and
 * whether it holds a non-finite value: the column's own are those of the segments it holds, so after
 * slg_index_remove_segment a histogram's dense id range is what a fresh registration over the segments left
 * gives.  The reference's behaviour on NaN / +-inf is an accident of `as i64` saturation and f64::min: a batch
 * that names such a column fails with SLG_ERR_UNSUPPORTED (CPU path).
 * A keyword column holds u32 ordinals into ONE caller-owned dictionary of n_ords keys: the caller maps each
 * segment's own dictionary (index/fastfields.rs:711-734) to global ordinals; an ordinal >= n_ords is
 * SLG_ERR_INVALID.  Return the field id (>= 0) or a negative error code. */
#define SLG_MAX_AGGS 8u          /* nodes of one spec, roots and children together */
#define SLG_MAX_AGG_RANGES 16u   /* ranges of one SLG_AGG_RANGE node */
#define SLG_MAX_AGG_CELLS 65536u /* count cells + stats cells of one query */
#define SLG_AGG_LDS_BYTES 32768u /* tables of 4 B per count cell + 32 B per stats cell up to this size are
                                    filled in LDS, larger ones in device memory (same results) */
#define SLG_MAX_AGG_SCRATCH_WORDS (1u << 19) /* u32 words of one query's value-node scratch (2 MB): the cardinality
                                               bitmaps plus the fine tables of the percentiles nodes */
#define SLG_AGG_PCT_LDS_BYTES 16384u /* of SLG_AGG_LDS_BYTES, held back by a spec with a percentiles node: its
                                        coarse histogram, then its fine tables when they fit */
#define SLG_MAX_AGG_RANKS (1u << 24) /* distinct values of a ranked column (slg_index_rank_agg_field) */
enum { SLG_AGG_TERMS = 0, SLG_AGG_HISTOGRAM = 1, SLG_AGG_RANGE = 2, SLG_AGG_STATS = 3,
       SLG_AGG_CARDINALITY = 4, SLG_AGG_PERCENTILES = 5, SLG_AGG_PERCENTILE_RANKS = 6,
       /* (7 is not a kind) */
       SLG_AGG_DATE_HISTOGRAM = 8, SLG_AGG_FILTER = 9 };
/* slg_agg_node.calendar_unit */
enum { SLG_DATE_FIXED = 0, SLG_DATE_DAY = 1, SLG_DATE_WEEK = 2, SLG_DATE_MONTH = 3, SLG_DATE_QUARTER = 4,
       SLG_DATE_YEAR = 5 };
int slg_index_add_agg_field_f64(slg_index *index, const uint32_t *const *seg_offsets,
                                const double *const *seg_values);
int slg_index_add_agg_field_i64(slg_index *index, const uint32_t *const *seg_offsets,
                                const int64_t *const *seg_values);
int slg_index_add_agg_field_ord(slg_index *index, const uint32_t *const *seg_offsets,
                                const uint32_t *const *seg_ords, uint32_t n_ords);
/* Batches already prepared with the field keep its columns (they belong to the batch's index state). */
int slg_index_remove_agg_field(slg_index *index, int agg_field_id);
/* The value ranks of a registered column, what SLG_AGG_CARDINALITY and SLG_AGG_PERCENTILES need of a numeric
 * field.  Builds the field's value dictionary — the sorted distinct values over all segments, ordered and told
 * apart by the order-preserving u64 key of their bits (so -0.0 and 0.0 are two entries, as the reference hashes
 * to_bits(), aggs/mod.rs:1549) — and, beside each segment's values, a u32 rank array with the same indexing.
 * Returns the distinct count R (>= 0) or a negative error code; a second call returns R and does nothing else; a
 * keyword field returns n_ords (its ordinals are its ranks).  Cost on the device: 4 B per value + 8 B per distinct
 * value; the dictionary is kept on the host too (prepare looks `missing` up in it).  The values are sorted on the
 * host: registration is not the hot path.  A new index state, as every update: slg_index_update_deleted keeps the
 * ranks, slg_index_remove_segment drops that segment's and keeps the dictionary (then a superset: harmless).
 * SLG_ERR_UNSUPPORTED: a column with a non-finite value; an _i64 column with a value beyond +-2^53 (two i64 values
 * the reference counts apart became one f64); R > SLG_MAX_AGG_RANKS. */
int64_t slg_index_rank_agg_field(slg_index *index, int agg_field_id);

/* One aggregation node.  A node is a root (parent == -1) or the child of an EARLIER bucket root (terms,
 * histogram, range, date_histogram or filter); children have no children.  A child under a bucket collects the doc once per parent
 * bucket the doc was counted in (aggs/mod.rs:905-908, 1026-1028, 1200-1202).
 *   SLG_AGG_TERMS      keyword column.  A doc counts once in every DISTINCT ordinal it holds (:898-909); a
 *                      doc without a value counts in row missing_ord if has_missing (:914-929).  missing_ord
 *                      in [0, n_ords]: n_ords = a key of its own (one more row), a smaller value = the missing
 *                      key equals that real key (the reference puts both into one bucket).
 *   SLG_AGG_HISTOGRAM  numeric column.  Bucket id = floor((val - offset) / interval) in IEEE f64 (:1162-1164);
 *                      a doc counts once per DISTINCT id (:1174-1184); with has_hard_bounds values with
 *                      val < hard_min || val > hard_max are skipped (:1176-1180); a doc without a value has the
 *                      one value `missing` if has_missing (:597-610).  interval > 0 and finite, offset finite.
 *   SLG_AGG_RANGE      numeric column, n_ranges <= SLG_MAX_AGG_RANGES.  A doc counts once in EVERY range for
 *                      which ANY of its values has from <= val && val <= to (:1019-1030: `to` is inclusive);
 *                      an absent bound is -/+infinity; `missing` as above.
 *   SLG_AGG_STATS      numeric column: count, min, max, sum over EVERY value of every collected doc (:1426-1441);
 *                      `missing` as above.  value_count, min, max, sum and avg follow on the host; extended_stats
 *                      (m2) is not built.
 *   SLG_AGG_DATE_HISTOGRAM numeric column; a bucket root like the three above (root, or child of a bucket root;
 *                      parent of every kind that can be a child).  The doc's values (`missing` as above) are
 *                      taken `as i64`, which truncates an f64 toward zero (-0.5 -> 0, -1.5 -> -1) (:1320-1328);
 *                      with has_hard_bounds a value with val < date_hard_min || val > date_hard_max (i64, both
 *                      ends inclusive) is skipped (:1334-1338); a doc counts once per DISTINCT bucket and its
 *                      children collect once per bucket it was counted in (:1343-1360).  All times are i64
 *                      milliseconds.  calendar_unit SLG_DATE_FIXED: id = ceil((val - date_offset) as f64 /
 *                      date_step as f64), ONE IEEE f64 division, then ceil (bucket_start, :3391-3396) — ceil, not
 *                      floor: a value on a boundary is its own bucket, any other goes to the NEXT boundary; key =
 *                      id * date_step + date_offset.  SLG_DATE_DAY .. _YEAR: t = val - date_offset lies in a UTC
 *                      proleptic-Gregorian day / ISO week (from Monday) / month / quarter / year
 *                      (truncate_calendar, :3410-3429); id = the unit's index since 1970 with floor semantics
 *                      (t = -1 is 1969-12-31): day floor(t / 86 400 000), week floor((day + 3) / 7), month
 *                      (y - 1970) * 12 + (m - 1), quarter floor(month / 3), year y - 1970; key = the unit's start
 *                      in ms + date_offset.  date_step is read for SLG_DATE_FIXED only.  The ids are dense: row i
 *                      of the table is id first_id + i.
 *   SLG_AGG_FILTER     no column (field is not read): ONE bucket that counts every collected doc whose bit in the
 *                      reject bitmap of the registered filter `filter` is clear (FilterCollector::collect,
 *                      :1664-1674; a filter without a bitmap for a segment rejects nothing there); a bucket root
 *                      like date_histogram: its children collect the docs that pass.  Any registered filter id
 *                      serves: bitmaps, ranges, term filters and filter trees alike.
 * Value nodes: order and identity questions over the values of the collected docs, answered from the value ranks
 * of the column (slg_index_rank_agg_field) into a table of 8-byte cells (slg_batch_fetch_agg_values):
 *   SLG_AGG_CARDINALITY      keyword or RANKED numeric column: the number of distinct values over every value of
 *                      every collected doc (:1508-1556; exact, a HashSet — precision_threshold is carried but
 *                      never used, :2688-2692).  A doc without a value contributes `missing` if has_missing: the
 *                      key missing_ord of a keyword column as for terms, the f64 `missing` of a numeric one
 *                      (its rank when the dictionary holds it, one rank beyond R otherwise).  Root, or child of a
 *                      bucket root: one set per parent bucket the doc was counted in.  Table: parent_rows x 1.
 *   SLG_AGG_PERCENTILES      RANKED numeric column, ROOT ONLY (as a child: SLG_ERR_UNSUPPORTED).  percents in
 *                      from[0 .. n_ranges), 1 <= n_ranges <= SLG_MAX_AGG_RANGES.  Over the sorted multiset vals of
 *                      every value (`missing` as above) with n elements: rank = (clamp(p, 0, 100) / 100) * (n - 1)
 *                      in IEEE f64, low = floor, high = ceil (:529-532).  Table: 1 x (1 + 2 * n_ranges): n, then
 *                      per percent the bits of vals[low] and vals[high].  The host returns vals[low] when low ==
 *                      high, else vals[low] * (1 - w) + vals[high] * w with w = rank - low (:533-537); 0.0 when
 *                      n == 0 (:523-525).  A `missing` the dictionary does not hold takes a virtual rank at its
 *                      lower bound (the ranks at or above it shift by one): no dictionary is rebuilt per batch.
 *   SLG_AGG_PERCENTILE_RANKS numeric column (ranks not needed), targets in from[0 .. n_ranges).  Table:
 *                      parent_rows x (1 + n_ranges): n, then per target the count of values <= target (:552).
 *                      The host returns count / max(n, 1) * 100, 0.0 when n == 0 (:548-553).  Root or child.
 * ANOTHER DELIBERATE DEVIATION: the reference's quantiles are exact up to PERCENTILE_EXACT_LIMIT = 256 values
 * and a t-digest estimate beyond (:472-545).  The device is exact at any n: it equals the reference where the
 * reference is exact and is never further from the truth elsewhere.
 * Everything after the tables is the caller's: ordering terms buckets (count desc, key string asc), size,
 * min_doc_count, extended_bounds, histogram keys id * interval + offset, pipeline aggregations.
 *
 * ONE DELIBERATE DEVIATION: the reference truncates terms buckets to shard_size / size and applies
 * min_doc_count PER SEGMENT before it merges (:932-944, 1230-1232, 2368-2393), so its multi-segment counts can
 * be too low.  The device counts over all segments and is exact; it equals the reference whenever no segment
 * truncates or drops a bucket.
 *
 * Determinism: counts, min and max are exact and identical from run to run.  sum is accumulated with f64
 * atomic adds in an order the hardware picks: its last bits may differ between runs when the values are not
 * exactly summable. */
typedef struct {
  int32_t kind;             /* SLG_AGG_* */
  int32_t field;            /* agg field id */
  int32_t parent;           /* -1, or the index of an earlier bucket root */
  uint32_t has_missing;
  double missing;           /* numeric kinds */
  uint32_t missing_ord;     /* SLG_AGG_TERMS */
  uint32_t has_hard_bounds; /* SLG_AGG_HISTOGRAM */
  double interval, offset, hard_min, hard_max;
  uint32_t n_ranges;        /* SLG_AGG_RANGE; the percents / targets of SLG_AGG_PERCENTILES / _PERCENTILE_RANKS */
  double from[SLG_MAX_AGG_RANGES], to[SLG_MAX_AGG_RANGES]; /* (percents and targets: from[]) */
  uint32_t calendar_unit;   /* SLG_AGG_DATE_HISTOGRAM: SLG_DATE_* */
  int32_t filter;           /* SLG_AGG_FILTER: a registered filter id */
  /* SLG_AGG_DATE_HISTOGRAM, i64 milliseconds (`missing` stays the f64 member above: the reference hands it to
   * numeric_values as an f64 and takes it `as i64` again; has_hard_bounds says whether the two bounds are read) */
  int64_t date_step, date_offset, date_hard_min, date_hard_max;
} slg_agg_node;
typedef struct {
  uint32_t n_nodes; /* 1 .. SLG_MAX_AGGS */
  slg_agg_node nodes[SLG_MAX_AGGS];
} slg_agg_spec;
/* A node's table is parent_rows x rows, parent-major (parent_rows = 1 for a root, else the parent's rows).
 * rows: terms n_ords (+ 1 when missing_ord == n_ords); histogram the dense id range that the column's finite
 * minimum and maximum, `missing` and the hard bounds allow (the bucket formula is monotone), row i = id
 * first_id + i; date_histogram the same over its ids (an empty range: one row that is never counted); filter 1;
 * range n_ranges; stats 1; cardinality 1; percentile_ranks 1 + n_ranges; percentiles
 * 1 + 2 * n_ranges.  offset: the table's first cell in the query's count table (bucket kinds), stats table
 * (is_stats == 1) or value table (is_stats == 2). */
typedef struct {
  uint32_t parent_rows, rows;
  int64_t first_id; /* histogram, date_histogram: the id of row 0; else 0 */
  uint32_t is_stats; /* 0 count table, 1 stats table, 2 value table */
  uint64_t offset;
} slg_agg_layout;
typedef struct {
  uint64_t count;
  double min, max, sum; /* all zero when count == 0 (StatsState::default) */
} slg_agg_stats;
/* slg_batch_prepare_plans (sort_or_null == NULL: score order) or slg_batch_prepare_sorted with one
 * aggregation spec for the whole batch.  Every query shape those two take is accepted; the batch runs through
 * slg_batch_run / _fetch / _matched_counts as any sorted batch.  Checked before anything else, without an
 * index: aggs NULL, n_nodes == 0, an unknown kind, a parent that is not an earlier bucket root, a
 * non-positive or non-finite interval, a non-finite offset / missing, a NaN bound, percent or target,
 * n_ranges == 0 (range, percentiles, percentile_ranks): SLG_ERR_INVALID; n_nodes > SLG_MAX_AGGS, n_ranges >
 * SLG_MAX_AGG_RANGES or a percentiles node with a parent: SLG_ERR_UNSUPPORTED.  A date_histogram node:
 * calendar_unit > SLG_DATE_YEAR or a fixed date_step < 1: SLG_ERR_INVALID; |date_offset|, |missing| or a hard bound
 * beyond 2^53: SLG_ERR_UNSUPPORTED.  A filter node with filter < 0: SLG_ERR_INVALID.  Against
 * the index: a date_histogram node on a keyword column, or a filter id that is not registered in the batch's index
 * state (never registered, or removed): SLG_ERR_INVALID; a date_histogram column that holds a value beyond +-2^53, or,
 * under a calendar unit, a collectable val - date_offset outside 0001-01-01T00:00:00Z .. 9999-12-31T23:59:59.999Z
 * (-62 135 596 800 000 .. 253 402 300 799 999 ms): SLG_ERR_UNSUPPORTED (CPU path; within these limits `as i64`,
 * `as f64` and val - offset are exact and cannot overflow).  For every kind: an unknown field id, a field
 * without a column for every segment, a field of the wrong kind for its node, missing_ord > n_ords, a numeric field without ranks under a cardinality or percentiles node
 * (slg_index_rank_agg_field): SLG_ERR_INVALID; a numeric column with a non-finite value, more than
 * SLG_MAX_AGG_CELLS cells per query (value cells count too), or more than SLG_MAX_AGG_SCRATCH_WORDS words of
 * value-node scratch per query (parent_rows x ceil(ranks / 32) per cardinality node, plus the fine tables of a
 * percentiles node: min(32, 2 * n_ranges) << max(0, ceil_log2(ranks) - 12) when that shift is > 0):
 * SLG_ERR_UNSUPPORTED.  Aggregations behind a clause or score stage: slg_batch_prepare_request, "compound requests" below.
 * Aggregations are not built on cursor, hybrid,
 * vector-only, sharded or coalesced batches (slg_batch_run_sharded* refuses an aggregation batch:
 * SLG_ERR_UNSUPPORTED). */
slg_batch *slg_batch_prepare_aggs(slg_index *index, uint32_t nq, const uint32_t *q_offsets,
                                  const uint32_t *q_term_ids, const float *q_weights,
                                  const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                                  const slg_sort_spec *sort_or_null, const slg_agg_spec *aggs, uint32_t k,
                                  int strategy);
/* The layout of every node's table (out: n_nodes entries).  The cells of one query's count table
 * (count_cells) and stats table (stats_cells) are the sums of parent_rows * rows over the bucket nodes and
 * over the stats nodes; tables lie in node order. */
int slg_batch_agg_layout(const slg_batch *batch, slg_agg_layout *out);
/* The tables of the batch's last run: counts [nq x count_cells], stats [nq x stats_cells] (either may be
 * NULL when it has no cells); waits for the batch.  A composite batch (slg_batch_prepare_composite) has the
 * composite's cells behind the spec's in every query's row: see slg_batch_composite_layout. */
int slg_batch_fetch_aggs(slg_batch *batch, uint64_t *counts, slg_agg_stats *stats);
/* The value tables of the batch's last run: values [nq x value_cells], value_cells = the sum of parent_rows * rows
 * over the value nodes (is_stats == 2), in node order; waits for the batch.  Counts, n and the percentile cells
 * (bits of an f64) are exact and identical from run to run: nothing here depends on an order. */
int slg_batch_fetch_agg_values(slg_batch *batch, uint64_t *values);
/* One-shot form: slg_search_batch_sorted with an aggregation spec (sort_or_null == NULL: score order);
 * counts / stats are sized by the caller from the spec (a prepared batch tells through
 * slg_batch_agg_layout); out_matched ([nq]) may be NULL. */
int slg_search_batch_aggs(slg_index *index, const slg_query *queries, uint32_t nq,
                          const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                          const slg_sort_spec *sort_or_null, const slg_agg_spec *aggs, uint32_t k, int strategy,
                          uint32_t *out_doc, uint32_t *out_seg, float *out_score, uint32_t *out_count,
                          uint64_t *out_matched, uint64_t *counts, slg_agg_stats *stats);
/* slg_search_batch_aggs with the value tables (values: [nq x value_cells], may be NULL without value nodes).
 * slg_search_batch_aggs itself refuses a spec with value nodes (SLG_ERR_INVALID): it has nowhere to put them. */
int slg_search_batch_agg_values(slg_index *index, const slg_query *queries, uint32_t nq,
                                const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                                const slg_sort_spec *sort_or_null, const slg_agg_spec *aggs, uint32_t k,
                                int strategy, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                                uint32_t *out_count, uint64_t *out_matched, uint64_t *counts, slg_agg_stats *stats,
                                uint64_t *values);

/* ---- top_hits aggregation: the best hits per bucket ---------------------------------------------------
 * TopHitsAggregation (api/types.rs:969-980; TopHitsCollector, query/aggs/mod.rs:1870-1981): per list — the whole
 * matched set for a root node, every bucket of its parent for a child — the limit = from + size best matched docs
 * under the node's sort are kept and the rows [from, from + size) of them reported, best first.  The order is the
 * field-sorted select's SortKey: parts in order, a Missing value after every value in both orders, ties by segment
 * then doc (query/sort.rs:80-123); an empty sort is `_score` desc.  A hit's score, and the value of a `_score`
 * part, is what the batch's rows carry for the same doc: the BM25 score in score order or under a batch sort with
 * a `_score` part, 0.0 under a field sort without one (ScoreMode::MatchOnly).  A child sees a doc once per parent
 * bucket the doc was counted in.  `fields` and `highlight_field` are doc-store work on the finished hits and stay
 * with the caller: the device returns (segment, doc, score).
 *
 * slg_agg_node does not grow: top_hits nodes travel in a spec of their own, next to the aggregation spec.
 * slg_batch_prepare_top_hits is slg_batch_prepare_aggs plus that spec; aggs_or_null may be NULL only when every
 * node is a root.  Rows, matched counts and every aggregation table of such a batch are bit-identical to the same
 * batch prepared with slg_batch_prepare_aggs (without aggs: with slg_batch_prepare_plans / _sorted), and
 * slg_batch_matched_counts serves it.  Checked before the index is looked at (after the aggregation spec's own
 * checks): top_hits NULL, n_nodes == 0, a parent that is neither -1 nor the index of a ROOT bucket node (terms,
 * histogram, range, date_histogram, filter) of aggs — a parent that is itself a child, a third level, is
 * SLG_ERR_UNSUPPORTED —, aggs NULL with a child node, an order that is neither SLG_ORDER_ASC nor _DESC, a sort
 * field id below SLG_SORT_SCORE: SLG_ERR_INVALID; n_nodes > SLG_MAX_TOP_HITS_NODES, size == 0 (nothing to select:
 * the total is in the tables already), from + size > SLG_MAX_TOP_HITS, more than SLG_MAX_SORT_PARTS parts:
 * SLG_ERR_UNSUPPORTED (the CPU path; a keyword sort field cannot be registered, as for slg_batch_prepare_sorted).
 * Against the index: an unknown sort field id or one without a column for every segment: SLG_ERR_INVALID; more
 * than SLG_MAX_TOP_HITS_CELLS hit cells per query (the sum of lists x size: a parent's rows are known only there):
 * SLG_ERR_UNSUPPORTED.  Nodes may come in any order; nodes of one parent that follow one another share its bucket
 * runs, otherwise each builds them again (the same lists, more time).  Memory per batch: nq x (8 B x max_entries + 12 B x hit_cells + 4 B x list_cells), plus 4 B
 * per row of a parent of more than 4096 rows.  Not built (the CPU path): cursor, hybrid, vector-only, scan, sharded
 * and coalesced batches (no such entry point takes the spec; behind a clause or score stage:
 * slg_batch_prepare_request, "compound requests" below; slg_batch_run_sharded* refuses the batch), a third
 * level, from + size > 64, keyword sort parts. */
#define SLG_MAX_TOP_HITS_NODES 4u
#define SLG_MAX_TOP_HITS 64u              /* from + size of one node: one entry per lane */
#define SLG_MAX_TOP_HITS_CELLS 65536u     /* hit cells of one query: sum of lists x size */
#define SLG_MAX_TOP_HITS_ENTRIES (1u << 19) /* bucket-run entries of one query (default capacity) */
typedef struct {
  int32_t parent;        /* -1 = root, else the index of a ROOT bucket node of the aggs spec */
  uint32_t from, size;
  slg_sort_spec sort;    /* n_parts == 0: _score desc */
} slg_top_hits_node;
typedef struct {
  uint32_t n_nodes;      /* 1 .. SLG_MAX_TOP_HITS_NODES */
  uint32_t max_entries;  /* 0 = SLG_MAX_TOP_HITS_ENTRIES; smaller: less memory per query */
  slg_top_hits_node nodes[SLG_MAX_TOP_HITS_NODES];
} slg_top_hits_spec;
typedef struct {
  uint32_t lists;        /* 1 for a root, else the parent's rows */
  uint32_t size;
  uint32_t list_offset;  /* first list of the node in a query's count array */
  uint32_t hit_offset;   /* first hit cell of the node in a query's hit arrays */
} slg_top_hits_layout;
slg_batch *slg_batch_prepare_top_hits(slg_index *index, uint32_t nq, const uint32_t *q_offsets,
                                      const uint32_t *q_term_ids, const float *q_weights,
                                      const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                                      const slg_sort_spec *sort_or_null, const slg_agg_spec *aggs_or_null,
                                      const slg_top_hits_spec *top_hits, uint32_t k, int strategy);
/* One entry per top_hits node (out: n_nodes entries).  A node's hits are lists x size cells: list-major, in node
 * order, lists in the parent's row order.  hit_cells of a query = the sum of lists x size, list_cells = the sum of
 * lists. */
int slg_batch_top_hits_layout(const slg_batch *batch, slg_top_hits_layout *out);
/* The lists of the batch's last run: out_doc, out_seg, out_score [nq x hit_cells], out_count [nq x list_cells],
 * out_status [nq] (any may be NULL); waits for the batch.  out_count[list] = min(size, max(0, collected - from))
 * real hits, cells past it are zero.  A list's total is not returned here: it is the parent's count cell for a
 * child (slg_batch_fetch_aggs) and the matched count for a root (slg_batch_matched_counts).  Status 0: ok; 1: the
 * query needed more than max_entries bucket-run entries (the sum of a parent's count row): its lists are all
 * zero and the caller takes that request to the CPU path; the batch's rows, matched counts and aggregation tables
 * are unaffected.  Nothing here depends on scheduling: the key is a total order.  SLG_ERR_INVALID on a batch of
 * another kind. */
int slg_batch_fetch_top_hits(slg_batch *batch, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                             uint32_t *out_count, uint32_t *out_status);
/* One-shot form: slg_search_batch_agg_values with a top_hits spec (aggs_or_null as above; counts / stats / values
 * may be NULL without cells of their kind); the th_ arrays are sized by the caller as slg_batch_top_hits_layout
 * would tell. */
int slg_search_batch_top_hits(slg_index *index, const slg_query *queries, uint32_t nq,
                              const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                              const slg_sort_spec *sort_or_null, const slg_agg_spec *aggs_or_null,
                              const slg_top_hits_spec *top_hits, uint32_t k, int strategy, uint32_t *out_doc,
                              uint32_t *out_seg, float *out_score, uint32_t *out_count, uint64_t *out_matched,
                              uint64_t *counts, slg_agg_stats *stats, uint64_t *values, uint32_t *th_doc,
                              uint32_t *th_seg, float *th_score, uint32_t *th_count, uint32_t *th_status);

/* ---- composite aggregation: ordered key tuples, paged -----------------------------------------------
 * CompositeAggregation (api/types.rs:694-718; CompositeCollector and finalize_composite, query/aggs/mod.rs:
 * 1689-1842, 3264-3368): the bucket space is the cross product of the sources' key spaces, and a request returns
 * the `size` smallest tuples above `after`.  A source is a keyword column (terms: the dictionary string, in UTF-8
 * byte order) or an f64 column (histogram: floor(v / interval) * interval in IEEE f64, identity by bits, order
 * total_cmp, so -0.0 and 0.0 are two buckets).  A doc without a value in any one source is skipped; otherwise it
 * is counted once in every distinct tuple of its values.  Segments merge by key without truncation, so the device's
 * all-segment counts are the reference's.
 *
 * Packed key: a tuple is ONE u64, source 0 in the most significant bits; part i is a slot number < slots[i] in
 * bits[i] = ceil_log2(slots[i]) bits at `shift`.  A terms slot is ord_rank[ord].  Histogram slots run over the ids
 * floor(vmin / interval) .. floor(vmax / interval) of the column's recorded finite minimum and maximum, with ONE
 * extra slot for -0.0 when id 0 is in the range: zero_slot is the slot of -0.0 (= -first_id), the slot of id 0
 * (+0.0) is zero_slot + 1, and every positive id is shifted by one.  A column without a value has one slot that is
 * never emitted.  Integer order of the key is the reference's tuple order; key_bits <= 63, ~0 is the empty marker.
 *
 * slg_batch_prepare_composite is slg_batch_prepare_aggs plus the spec (aggs_or_null may be NULL).  Rows, matched
 * counts and every table of aggs_or_null are bit-identical to the same batch without the composite.  The composite's
 * `size` count cells, then its children's tables (parent_rows = size), lie behind the cells of aggs_or_null in the
 * arrays of slg_batch_fetch_aggs: a query's count row is count_cells(aggs) + composite count cells wide, its stats
 * row likewise.  Checked before the index is looked at (after the aggregation spec's own checks): spec NULL,
 * n_sources == 0, an unknown source kind, a non-positive or non-finite interval, a child that slg_batch_prepare_aggs
 * would reject as a root: SLG_ERR_INVALID; n_sources > SLG_MAX_COMPOSITE_SOURCES, size == 0 (the response is empty:
 * the caller answers it), size > SLG_MAX_COMPOSITE_SIZE, n_children > SLG_MAX_AGGS, a cardinality, percentiles or
 * percentile_ranks child: SLG_ERR_UNSUPPORTED.  Against the index: an unknown field, a field without a column for
 * every segment, a field of the wrong kind for its source, an ord_rank that is not a permutation of [0, n_ords):
 * SLG_ERR_INVALID; a histogram column with a non-finite value, one registered with slg_index_add_agg_field_i64 (the
 * reference reads f64 columns only and skips every doc: the caller answers the empty response), one with an id at or
 * beyond +-2^31, key_bits > 63, size x (1 + child cells) plus the cells of aggs_or_null over SLG_MAX_AGG_CELLS:
 * SLG_ERR_UNSUPPORTED.  Memory per batch: nq x 8 B x (size + 1) keys, the table cells, 4 B per ordinal of a ranked
 * terms source.  Not built (the CPU path): composite on scan, cursor, hybrid, vector-only, sharded
 * (slg_batch_run_sharded* refuses the batch) or coalesced batches (behind a clause or score stage:
 * slg_batch_prepare_request, "compound requests" below); top_hits or value nodes under a composite;
 * `sampling`; more than one composite per request; a composite below another aggregation; `missing`, `offset` or
 * bounds on a source (the reference has none). */
#define SLG_MAX_COMPOSITE_SOURCES 4u
#define SLG_MAX_COMPOSITE_SIZE 1024u
enum { SLG_COMPOSITE_TERMS = 0, SLG_COMPOSITE_HISTOGRAM = 1 };
typedef struct {
  uint32_t kind;   /* SLG_COMPOSITE_* */
  int32_t field;   /* a registered aggregation column */
  double interval; /* histogram */
  const uint32_t *ord_rank; /* terms: [n_ords] permutation, the rank of each ordinal's key in byte order;
                               NULL = the ordinals already are in key order */
} slg_composite_source;
typedef struct {
  uint32_t n_sources, size;
  slg_composite_source sources[SLG_MAX_COMPOSITE_SOURCES];
  uint32_t n_children;
  slg_agg_node children[SLG_MAX_AGGS]; /* parent is not read: every child is a child of the composite */
} slg_composite_spec;
typedef struct {
  uint32_t shift, bits;
  uint64_t slots;
  int64_t first_id;  /* histogram: the id of slot 0 */
  int64_t zero_slot; /* histogram: the slot of -0.0 (the slot of +0.0 follows it); -1 when id 0 is outside the range */
} slg_composite_source_layout;
typedef struct {
  uint32_t n_sources, size, key_bits, n_children;
  slg_composite_source_layout sources[SLG_MAX_COMPOSITE_SOURCES];
  uint64_t count_offset; /* the composite's `size` count cells in a query's count row */
  slg_agg_layout children[SLG_MAX_AGGS]; /* parent_rows = size; offsets into a query's count / stats row */
} slg_composite_layout;
slg_batch *slg_batch_prepare_composite(slg_index *index, uint32_t nq, const uint32_t *q_offsets,
                                       const uint32_t *q_term_ids, const float *q_weights,
                                       const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                                       const slg_sort_spec *sort_or_null, const slg_agg_spec *aggs_or_null,
                                       const slg_composite_spec *composite, uint32_t k, int strategy);
int slg_batch_composite_layout(const slg_batch *batch, slg_composite_layout *out);
/* Per query an INCLUSIVE lower bound in packed key space for the runs that follow (copied; NULL or 0: from the
 * start; a bound >= 1 << key_bits: no bucket).  One prepared batch pages through a bucket set with set-after + run. */
int slg_batch_set_composite_after(slg_batch *batch, const uint64_t *q_lower_or_null);
/* The selection of the batch's last run: keys [nq x size] ascending, n_buckets [nq], has_more [nq] (any may be
 * NULL); waits for the batch.  Row r of a query's composite count cells and of every child table belongs to
 * keys[r]; rows past n_buckets are zero.  Keys, n_buckets, has_more and counts are exact and the same on every
 * run; a child's sum carries the tolerance of every stats sum.  SLG_ERR_INVALID on a batch of another kind. */
int slg_batch_fetch_composite(slg_batch *batch, uint64_t *keys, uint32_t *n_buckets, uint32_t *has_more);
/* One-shot form for the first page (no lower bound): slg_search_batch_aggs with a composite spec; counts / stats
 * are sized by the caller as slg_batch_agg_layout and slg_batch_composite_layout would tell. */
int slg_search_batch_composite(slg_index *index, const slg_query *queries, uint32_t nq,
                               const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                               const slg_sort_spec *sort_or_null, const slg_agg_spec *aggs_or_null,
                               const slg_composite_spec *composite, uint32_t k, int strategy, uint32_t *out_doc,
                               uint32_t *out_seg, float *out_score, uint32_t *out_count, uint64_t *out_matched,
                               uint64_t *counts, slg_agg_stats *stats, uint64_t *cp_keys, uint32_t *cp_n_buckets,
                               uint32_t *cp_has_more);

/* ---- significant_terms and rare_terms: select a keyword's buckets ------------------------------------
 * SignificantTermsAggregation and RareTermsAggregation (api/types.rs:875-901; SignificantTermsCollector,
 * RareTermsCollector, compute_background_counts, the merge and finalize: query/aggs/mod.rs:131-359, 2110-2181,
 * 2395-2424, 2515-2595).  Both kinds count a collected doc once per DISTINCT value of a keyword column (no
 * `missing`) and return at most `size` buckets.
 *   significant: buckets with doc_count >= max(min_doc_count, 1); the `size` with the highest count (count desc, key
 *     byte order asc) are kept, scored and returned by (score desc, count desc, key asc): the set is picked by count
 *     and ordered by score.  score = (doc_count_b / doc_count) / (bg_count_b / bg_count), three IEEE f64 divisions,
 *     0.0 when doc_count, bg_count or bg_count_b is zero.  doc_count (the node's): collected docs with a value.
 *     bg_count (the node's): over EVERY segment, the docs that are not deleted and pass background_filter, with a
 *     value or without.  bg_count_b: the sum, over the segments IN WHOSE FOREGROUND THE KEY OCCURS (the query
 *     collected a doc with that key there), of the docs of that segment that are not deleted, pass the filter and
 *     hold the key.  It is not the key's global background count: it is what the reference's merge adds up.
 *   rare: buckets with 1 <= doc_count <= max_doc_count, by (count asc, key asc), the first `size`.
 * The background comes from the registered column (bg_count_kernel at prepare, once per distinct (field, filter) of
 * the spec; the batch is pinned to its index state).
 *
 * Deliberate deviation (as for terms): the reference filters by the count bound and truncates to `size` per SEGMENT
 * and again after the merge; the device counts over all segments before it filters and truncates.  The two agree
 * whenever no segment drops or truncates a bucket that the merged answer would have needed: on one segment; for
 * significant_terms with min_doc_count <= 1 and `size` at least each segment's bucket count; for rare_terms when no
 * key is within max_doc_count in one segment and beyond it in the sum.  bg_count_b above is NOT part of the
 * deviation: it is the reference's sum exactly.
 *
 * slg_batch_prepare_term_buckets is slg_batch_prepare_aggs plus the spec (aggs_or_null may be NULL).  Rows, matched
 * counts and every table of aggs_or_null are bit-identical to the same batch without the spec.  A node WITH children
 * has `size` count cells (the rows' doc counts again, as a composite's) and then its children's tables (parent_rows =
 * size) behind the cells of aggs_or_null in the arrays of slg_batch_fetch_aggs, node after node; a node without
 * children has none.  Row r of a child table belongs to bucket r of slg_batch_fetch_term_buckets.
 * Checked before the index is looked at (after the aggregation spec's own checks): spec NULL, n_nodes == 0, an
 * unknown kind, a rare node with background_filter != -1, background_filter < -1, a child that slg_batch_prepare_aggs
 * would reject as a root: SLG_ERR_INVALID; n_nodes > SLG_MAX_TERM_BUCKET_NODES, size == 0 ("all buckets": the CPU
 * path), size > SLG_MAX_TERM_BUCKET_SIZE, n_children > SLG_MAX_AGGS, a cardinality, percentiles or percentile_ranks
 * child: SLG_ERR_UNSUPPORTED.  Against the index: an unknown field, a field without a column for every segment, a
 * numeric field, an unregistered filter id, an ord_rank that is not a permutation of [0, n_ords): SLG_ERR_INVALID;
 * more than SLG_MAX_AGG_CELLS cells of a query (per node n_ords foreground cells and n_ords background-sum cells,
 * with children size x (1 + child cells), plus the cells of aggs_or_null), or more than SLG_MAX_AGG_SCRATCH_WORDS
 * presence words of a query (a significant node: n_segs x ceil(n_ords / 32)): SLG_ERR_UNSUPPORTED.
 * Memory per batch: nq x 12 B per ordinal of every node, the presence words, nq x 36 B per output row, the child
 * cells; per distinct (field, filter): 4 B x n_segs x (n_ords + 1); 8 B per ordinal of a ranked node.
 * Not built (the CPU path; refused, or there is no entry point): `sampling`; `size` absent; a term-bucket node below
 * another aggregation; top_hits or value nodes below one; term buckets on scan, cursor, hybrid, vector-only,
 * sharded (slg_batch_run_sharded* refuses the batch) or coalesced batches (behind a clause or score stage:
 * slg_batch_prepare_request, "compound requests" below); together with a composite or
 * top_hits spec in one batch.  Pipeline children stay the caller's. */
#define SLG_MAX_TERM_BUCKET_NODES 4u
#define SLG_MAX_TERM_BUCKET_SIZE 1024u /* as SLG_MAX_COMPOSITE_SIZE */
enum { SLG_TERMS_SIGNIFICANT = 0, SLG_TERMS_RARE = 1 };
typedef struct {
  uint32_t kind;              /* SLG_TERMS_* */
  int32_t field;              /* a keyword column (slg_index_add_agg_field_ord) */
  uint32_t size;              /* 1 .. SLG_MAX_TERM_BUCKET_SIZE */
  uint64_t doc_count_bound;   /* significant: min_doc_count; rare: max_doc_count */
  int32_t background_filter;  /* significant: a registered filter id, -1 = none */
  const uint32_t *ord_rank;   /* as slg_composite_source.ord_rank; NULL = the ordinals are in key byte order */
  uint32_t n_children;
  slg_agg_node children[SLG_MAX_AGGS]; /* as slg_composite_spec.children */
} slg_term_bucket_node;
typedef struct {
  uint32_t n_nodes;
  slg_term_bucket_node nodes[SLG_MAX_TERM_BUCKET_NODES];
} slg_term_bucket_spec;
typedef struct {
  uint32_t size, n_children;
  uint64_t row_offset;   /* the node's first row in a query's rows of slg_batch_fetch_term_buckets */
  uint64_t count_offset; /* with children: the node's `size` count cells in a query's count row */
  slg_agg_layout children[SLG_MAX_AGGS]; /* parent_rows = size; offsets into a query's count / stats row */
} slg_term_bucket_node_layout;
typedef struct {
  uint32_t n_nodes;
  uint32_t rows; /* of one query: the sum of the nodes' sizes */
  slg_term_bucket_node_layout nodes[SLG_MAX_TERM_BUCKET_NODES];
} slg_term_bucket_layout;
slg_batch *slg_batch_prepare_term_buckets(slg_index *index, uint32_t nq, const uint32_t *q_offsets,
                                          const uint32_t *q_term_ids, const float *q_weights,
                                          const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                                          const slg_sort_spec *sort_or_null, const slg_agg_spec *aggs_or_null,
                                          const slg_term_bucket_spec *spec, uint32_t k, int strategy);
int slg_batch_term_buckets_layout(const slg_batch *batch, slg_term_bucket_layout *out);
/* The buckets of the batch's last run, in the response's final order: ords, doc_counts, bg_counts, score_bits (the
 * bits of the f64 score) [nq x rows], a node's rows at its row_offset; n_buckets, node_doc_count, node_bg_count
 * [nq x n_nodes] (any may be NULL); waits for the batch.  Rows past n_buckets are zero; for a rare node bg_counts,
 * score_bits and the two totals are zero.  Everything is exact and the same on every run.  SLG_ERR_INVALID on a
 * batch of another kind. */
int slg_batch_fetch_term_buckets(slg_batch *batch, uint32_t *ords, uint64_t *doc_counts, uint64_t *bg_counts,
                                 uint64_t *score_bits, uint32_t *n_buckets, uint64_t *node_doc_count,
                                 uint64_t *node_bg_count);
/* One-shot form: slg_search_batch_aggs with the spec; counts / stats are sized by the caller as slg_batch_agg_layout
 * and slg_batch_term_buckets_layout would tell. */
int slg_search_batch_term_buckets(slg_index *index, const slg_query *queries, uint32_t nq,
                                  const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                                  const slg_sort_spec *sort_or_null, const slg_agg_spec *aggs_or_null,
                                  const slg_term_bucket_spec *spec, uint32_t k, int strategy, uint32_t *out_doc,
                                  uint32_t *out_seg, float *out_score, uint32_t *out_count, uint64_t *out_matched,
                                  uint64_t *counts, slg_agg_stats *stats, uint32_t *tb_ords, uint64_t *tb_doc_counts,
                                  uint64_t *tb_bg_counts, uint64_t *tb_score_bits, uint32_t *tb_n_buckets,
                                  uint64_t *tb_node_doc_count, uint64_t *tb_node_bg_count);

/* ---- request coalescer ------------------------------------------------------------------------------
 * searchlite has no batch API: IndexReader::search takes one request (api/reader.rs:2539) and the HTTP
 * server gives every request its own blocking thread (searchlite-http/src/lib.rs:628-652).  The
 * coalescer turns concurrent single-query callers into batches: slg_coalescer_search blocks its caller
 * thread, the query joins the batch that is collecting (same k, strategy and segment count), the
 * coalescer's two dispatcher threads plan / run / fetch the batch on a HIP stream of its own while the next
 * batch already collects, and every caller returns with its own row — bit-identical to the same query in
 * slg_search_batch.  A batch closes when it holds max_batch queries, or max_wait_us after its first
 * query arrived; a query that finds the coalescer idle (nothing in flight) does not wait at all.
 * Thread-safe; out_doc / out_seg / out_score hold k entries, out_count one.
 *
 * A request is checked when it is submitted, before it joins a batch: whatever slg_batch_prepare_plan refuses
 * about one query — an unknown strategy or plan, k > SLG_MAX_K or more than SLG_MAX_QUERY_TERMS terms
 * (SLG_ERR_UNSUPPORTED), a tie outside [0, 1] or NaN, a leaf >= 2^31, a term id that is neither SLG_NO_TERM nor
 * below its segment's term count, a non-finite weight, a filter id that is not registered for every segment —
 * fails that request alone (SLG_ERR_INVALID unless noted), with its text in slg_coalescer_last_error, and costs
 * the callers that would have shared its batch nothing.  Two rules are stricter than the batch API's: a
 * non-finite weight is refused even where its term has no posting, and a negative filter id other than -1 is
 * refused.  A failure of the batch as a whole (the device, memory) goes to every caller of that batch.
 *
 * Up to 8 combinations of (k, strategy, segment count) collect at the same time.  A combination whose requests
 * have all been waited for gives its place to a new one, so any number of combinations may be used over the
 * coalescer's life; a request that meets 8 others with requests in flight at that moment fails with
 * SLG_ERR_UNSUPPORTED and may be sent again.
 *
 * Index updates need a quiesced coalescer: slg_index_add_segment / _remove_segment, and the removal of a filter
 * that requests name, must not run between a request's submit and its wait (a row is written at the width, and
 * checked against the segments and filters, of the index as it was at submit; the batch is planned on the index
 * as it is when the batch closes).  A request in flight across slg_index_update_deleted is answered from the
 * state before or after it.  Requests submitted after an update returns see the new index. */
typedef struct slg_coalescer slg_coalescer;
slg_coalescer *slg_coalescer_create(slg_index *index, uint32_t max_batch, uint32_t max_wait_us);
/* No caller may be inside slg_coalescer_search any more. */
void slg_coalescer_destroy(slg_coalescer *coalescer);
int slg_coalescer_search(slg_coalescer *coalescer, const slg_query *query, uint32_t k, int strategy,
                         uint32_t *out_doc, uint32_t *out_seg, float *out_score, uint32_t *out_count,
                         slg_stats *stats_or_null);
/* The same for a query with a flat score plan (slg_batch_prepare_plan: leaf[i] = leaf of query term i or
 * NULL, plan = SLG_PLAN_SUM | SLG_PLAN_DISMAX over the leaves, tie in [0, 1], n_leaves = leaves of the
 * plan or 0 = 1 + the largest leaf named) and / or a registered doc filter (filter_id, -1: none): what
 * an unmodified request over the default fields is (api/reader.rs:2576-2586).  Rows with and without
 * plans or filters share batches.  Two-level plans go through slg_batch_prepare_plans directly. */
int slg_coalescer_search_plan(slg_coalescer *coalescer, const slg_query *query, const uint32_t *leaf, int plan,
                              float tie, uint32_t n_leaves, int32_t filter_id, uint32_t k, int strategy,
                              uint32_t *out_doc, uint32_t *out_seg, float *out_score, uint32_t *out_count,
                              slg_stats *stats_or_null);
/* The two halves of slg_coalescer_search_plan, for callers that keep SEVERAL requests in flight per thread
 * (an async server task, a client that pipelines): slg_coalescer_submit puts the query into the collecting
 * batch and returns at once with a ticket; slg_coalescer_wait blocks until that batch's results are in,
 * copies the ticket's row out and gives the row back (every ticket must be waited for exactly once, by any
 * thread; the ticket is cleared).  slg_coalescer_poll: 1 if slg_coalescer_wait would not block, else 0.
 * The query's arrays may be reused as soon as submit returns.  A submit that fails took no ticket: there is
 * nothing to wait for.  want_stats != 0 asks for the request's slg_stats: slg_coalescer_wait writes
 * *stats_or_null — the slg_stats slg_batch_fetch reports for the same query — only for such a ticket and only when
 * it returns SLG_OK; for a ticket submitted with want_stats == 0, or on failure, *stats_or_null is left as it was.
 * A thread-per-request caller pays a sleep and
 * a wake-up per query — what bounds slg_coalescer_search on a host with few cores; with D tickets per
 * thread a thread sleeps at most once per D queries. */
typedef struct slg_ticket {
  void *batch;   /* opaque; NULL once waited for */
  uint32_t row, k, kind;
} slg_ticket;
int slg_coalescer_submit(slg_coalescer *coalescer, const slg_query *query, const uint32_t *leaf, int plan, float tie,
                         uint32_t n_leaves, int32_t filter_id, uint32_t k, int strategy, int want_stats,
                         slg_ticket *ticket);
int slg_coalescer_poll(const slg_coalescer *coalescer, const slg_ticket *ticket);
int slg_coalescer_wait(slg_coalescer *coalescer, slg_ticket *ticket, uint32_t *out_doc, uint32_t *out_seg,
                       float *out_score, uint32_t *out_count, slg_stats *stats_or_null);
/* Thread-local text of the last failure of slg_coalescer_search / _search_plan / _submit / _wait on this thread
 * (empty after a call that succeeded). */
const char *slg_coalescer_last_error(void);
/* Mean time (ms) a batch's leader spent collecting / in slg_batch_prepare / in set_stream + run / in
 * fetch + destroy, over the batches run so far. */
int slg_coalescer_phase_ms(const slg_coalescer *coalescer, double *collect, double *prepare, double *run,
                           double *fetch);
/* Batches run and queries served so far (their ratio = the mean batch size reached). */
int slg_coalescer_stats(const slg_coalescer *coalescer, uint64_t *n_batches, uint64_t *n_queries);

/* ---- index sharding over RCCL ------------------------------------------------------
 * The reference scores every segment independently and merges by (score desc, segment_ord asc,
 * doc asc) (api/reader.rs:2670-2778, query/sort.rs:80-93); with one shard of segments per GPU the
 * merge spans ranks.  A shard group ties this rank's index to an RCCL communicator: one process
 * (or host thread) per GPU creates its index over ITS segments and joins the group; rank 0 makes
 * the 128-byte id with slg_shard_unique_id and hands it to the other ranks out of band (the way
 * ncclGetUniqueId / ncclCommInitRank are used).  segs_per_rank = the largest shard's segment count:
 * a hit's segment ordinal in the merged result is rank * segs_per_rank + its local ordinal.
 * librccl is bound at run time; without it these calls fail with SLG_ERR_UNSUPPORTED. */
#define SLG_SHARD_UNIQUE_ID_BYTES 128u
typedef struct slg_shard_group slg_shard_group;
int slg_shard_unique_id(void *out, size_t out_bytes);
/* Collective: every rank of the group calls it (it returns when all have). */
slg_shard_group *slg_shard_group_create(slg_index *index, int rank, int world, const void *unique_id,
                                        uint32_t segs_per_rank);
void slg_shard_group_destroy(slg_shard_group *group);
/* slg_batch_run on this rank's segments, ONE ncclAllGather of the contiguous result blocks
 * ((3k+1) * Q * 4 bytes per rank) on the batch's stream, merge of the world's rows on the device.
 * Every rank prepares the SAME queries (same order, same k) and issues its sharded runs in the same
 * order.  out_* (host, [nq*k] / [nq]) receive the merged top-k on every rank; pass NULL for all four
 * to leave the result on the device (slg_batch_sharded_device_results) without waiting. */
int slg_batch_run_sharded(slg_batch *batch, slg_shard_group *group, uint32_t *out_doc, uint32_t *out_seg,
                          float *out_score, uint32_t *out_count);
/* Collectives on one communicator must be issued in the same order on every rank.  The group issues
 * them on a stream of its own, one at a time: slg_batch_run_sharded takes its turn in CALL order — so
 * every rank must call it for its batches in the same order, which one issuing thread per rank
 * guarantees (several batches may still be in flight, each on its own stream).  With several caller
 * threads per rank use the _seq form: `seq` numbers the sharded runs of the group 0, 1, 2, ... without
 * gaps, the SAME number for the same query batch on every rank; run `seq` issues its all-gather when
 * runs 0 .. seq-1 of this rank have issued theirs (a call may block until then; a failed run still
 * passes its turn on).  Do not mix the two forms on one group. */
int slg_batch_run_sharded_seq(slg_batch *batch, slg_shard_group *group, uint64_t seq, uint32_t *out_doc,
                              uint32_t *out_seg, float *out_score, uint32_t *out_count);
/* Passes the turn of run `seq` on without a collective: for a rank that could not prepare the batch of
 * that number (the runs behind it would wait for ever).  The other ranks must skip the same number —
 * an all-gather that one rank never joins does not complete. */
int slg_shard_group_skip_seq(slg_shard_group *group, uint64_t seq);
/* With slg_profile_enable on: device time (ms, summed) of the sharded runs FETCHED since the last call —
 * this rank's kernels, the all-gather (incl. waiting for the slowest rank), the merge — and their number.
 * Resets the sums. */
int slg_shard_group_stats(slg_shard_group *group, double *ms_kernels, double *ms_gather, double *ms_merge,
                          uint64_t *n_runs);
int slg_batch_sharded_device_results(slg_batch *batch, void **d_doc, void **d_seg, void **d_score,
                                     void **d_count);
/* Waits for the batch's sharded run and copies the merged top-k to host arrays (what
 * slg_batch_run_sharded does itself when given output arrays): lets a caller keep several sharded
 * batches in flight, each on its own stream, and collect them later. */
int slg_batch_fetch_sharded(slg_batch *batch, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                            uint32_t *out_count);

/*
 * Merge per-shard results gathered from several indexes/GPUs (device arrays, as produced
 * by slg_batch_device_results and concatenated shard-major: [n_shards][nq*k]) into the
 * global top-k by (score desc, shard_ord asc, segment asc, doc asc).  out_seg receives
 * shard_ord * seg_stride + seg.  All pointers are device pointers on `index`'s device.
 * k up to SLG_MAX_K, as the scorer (an index-sharded request with limit = 20 000 merges too).
 */
int slg_merge_shards_device(slg_index *index, uint32_t n_shards, uint32_t nq, uint32_t k,
                            const uint32_t *d_doc, const uint32_t *d_seg, const float *d_score,
                            const uint32_t *d_count, uint32_t seg_stride, uint32_t *d_out_doc,
                            uint32_t *d_out_seg, float *d_out_score, uint32_t *d_out_count);

/* ---- profiling hooks (bench.py roofline) -------------------------------------------- */

/* When enabled, every slg_batch_run brackets its scoring kernel with HIP events on the
 * launch stream. */
int slg_profile_enable(slg_index *index, int on);
/* Sum of scoring-kernel durations and number of launches since the last reset; waits
 * for the recorded events.  Resets the accumulators. */
int slg_profile_read(slg_index *index, uint32_t *n_launches, float *total_ms);

/* ---- rerank (fills gpu::rerank, gpu/rerank.rs:3) ------------------------------------- */

/*
 * For each query: candidates (cand_doc, cand_seg, cand_bm25)[cand_count[q] <= max_cand] ->
 * vector similarity against qvecs[q] (vectors/mod.rs:107-120: cosine = dot of
 * pre-normalized vectors, NaN -> 0; L2 = -sqrt(sum d^2)), blended as
 * compute_hybrid_score does for one clause (api/reader.rs:225-254; missing vector =>
 * -1.0 / f32::MIN, api/reader.rs:217-223), then top-k_out by (blended desc, seg asc, doc asc).
 * Host arrays in and out; blocks.
 */
int slg_rerank_batch(slg_index *index, uint32_t nq, const float *qvecs, const float *alpha,
                     const uint32_t *cand_doc, const uint32_t *cand_seg, const float *cand_bm25,
                     const uint32_t *cand_count, uint32_t max_cand, uint32_t k_out,
                     uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                     float *out_vec_score, uint32_t *out_count);

/* Same, all pointers device-resident and asynchronous on the index stream (chains after
 * slg_batch_run without a host round trip). */
int slg_rerank_batch_device(slg_index *index, uint32_t nq, const float *d_qvecs,
                            const float *d_alpha, const uint32_t *d_cand_doc,
                            const uint32_t *d_cand_seg, const float *d_cand_bm25,
                            const uint32_t *d_cand_count, uint32_t max_cand, uint32_t k_out,
                            uint32_t *d_out_doc, uint32_t *d_out_seg, float *d_out_score,
                            float *d_out_vec_score, uint32_t *d_out_count);

/* Rerank a batch's OWN device results (k candidates per query, as slg_batch_run left them) with
 * n_clauses vector clauses, asynchronously on the batch's stream: BM25 top-k -> rerank chains without a
 * host round trip and without leaving the batch's stream, so several such pipelines can be in flight
 * (slg_batch_set_stream).  Arguments as slg_rerank_multi_batch_device; n_clauses == 1 with d_boost ==
 * NULL takes the single-clause kernel. */
int slg_batch_rerank_device(slg_batch *batch, uint32_t n_clauses, const float *d_qvecs, const float *d_alpha,
                            const float *d_boost, uint32_t k_out, uint32_t *d_out_doc, uint32_t *d_out_seg,
                            float *d_out_score, float *d_out_vec_score, uint32_t *d_out_count);

/*
 * Hybrid rerank with several vector clauses over one candidate set (api/reader.rs:225-254;
 * n_clauses <= SLG_MAX_VECTOR_CLAUSES): qvecs[q][c][dim], alpha[q][c], boost[q][c] (NULL: 1.0; the
 * clause's similarity is multiplied by it, api/reader.rs:2421).  Blended score = mean over the
 * clauses of blend(alpha_c, bm25, vec_c); a candidate without a vector counts as -1.0 / f32::MIN in
 * every clause (:217-223); out_vec_score = sum of the clause similarities (:236-238).  All clauses
 * use the index's one vector field.  The [candidates x clauses] cosine products run on the f32
 * matrix cores (v_mfma_f32_16x16x4_f32).  n_clauses * (dim + 4 + max_cand) + 2 * max_cand floats
 * must fit the kernel's LDS budget (36 Ki floats), else SLG_ERR_UNSUPPORTED.
 */
/*
 * Vector fields beyond the one in slg_segment_desc (vectors/mod.rs:10-17: one VectorStore per
 * vector field).  Field 0 is the store of the segment descriptors; every call stages one more
 * field — one descriptor per segment of the index, vec_dim 0 where the segment has no vectors in
 * it — and returns its id (>= 1), or a negative error code.
 */
typedef struct {
  uint32_t vec_dim;            /* 0 => this segment has no vectors in the field */
  int32_t vec_metric;          /* SLG_METRIC_* */
  const uint32_t *vec_offsets; /* [n_docs] row index or SLG_NO_VECTOR */
  const float *vec_values;     /* [vec_rows * vec_dim] row-major */
  uint32_t vec_rows;
} slg_vector_field_desc;
int slg_index_add_vector_field(slg_index *index, const slg_vector_field_desc *per_segment, uint32_t n_segs);

/*
 * Hybrid rerank whose clauses name different vector fields (api/reader.rs:225-254: every clause has
 * its own field, metric and dimension).  clause_field[c] = field id of clause c (host array);
 * qvecs[q] = the clause vectors of query q one after another (sum of the clause dimensions
 * floats); alpha / boost [nq][n_clauses] as in slg_rerank_multi_batch.  A candidate without a
 * vector in clause c's field takes that clause's missing-vector score (-1.0 / f32::MIN by the
 * clause's metric); out_vec_score sums the clauses that found one.
 */
int slg_rerank_fields_batch(slg_index *index, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                            const float *qvecs, const float *alpha, const float *boost,
                            const uint32_t *cand_doc, const uint32_t *cand_seg, const float *cand_bm25,
                            const uint32_t *cand_count, uint32_t max_cand, uint32_t k_out, uint32_t *out_doc,
                            uint32_t *out_seg, float *out_score, float *out_vec_score, uint32_t *out_count);
int slg_rerank_fields_batch_device(slg_index *index, uint32_t nq, uint32_t n_clauses,
                                   const uint32_t *clause_field, const float *d_qvecs, const float *d_alpha,
                                   const float *d_boost, const uint32_t *d_cand_doc,
                                   const uint32_t *d_cand_seg, const float *d_cand_bm25,
                                   const uint32_t *d_cand_count, uint32_t max_cand, uint32_t k_out,
                                   uint32_t *d_out_doc, uint32_t *d_out_seg, float *d_out_score,
                                   float *d_out_vec_score, uint32_t *d_out_count);

int slg_rerank_multi_batch(slg_index *index, uint32_t nq, uint32_t n_clauses, const float *qvecs,
                           const float *alpha, const float *boost, const uint32_t *cand_doc,
                           const uint32_t *cand_seg, const float *cand_bm25, const uint32_t *cand_count,
                           uint32_t max_cand, uint32_t k_out, uint32_t *out_doc, uint32_t *out_seg,
                           float *out_score, float *out_vec_score, uint32_t *out_count);
int slg_rerank_multi_batch_device(slg_index *index, uint32_t nq, uint32_t n_clauses, const float *d_qvecs,
                                  const float *d_alpha, const float *d_boost, const uint32_t *d_cand_doc,
                                  const uint32_t *d_cand_seg, const float *d_cand_bm25,
                                  const uint32_t *d_cand_count, uint32_t max_cand, uint32_t k_out,
                                  uint32_t *d_out_doc, uint32_t *d_out_seg, float *d_out_score,
                                  float *d_out_vec_score, uint32_t *d_out_count);


/*
 * Exact vector-only search over every stored vector (search_vector_only, api/reader.rs:2187-2330).
 * Per query and clause c (field clause_field[c], host array; qvecs[q] = the clause vectors of query q
 * one after another, cosine vectors normalised by the caller): every doc that has a vector in the
 * field, is not deleted and passes the query's filter scores metric_similarity * boost[q][c]
 * (cosine: dot, NaN -> 0; L2: -sqrt(sum (x - y)^2)); the best cand_size by (score desc, segment asc,
 * doc asc) form the clause's list.  This is collect_vector_maps (:2379-2469) with the per-segment HNSW
 * search replaced by an exact scan, and with the filter applied before the truncation.  The docs of
 * any clause's list form the union; each scores compute_hybrid_score at bm25 = 0 (:225-254): a clause
 * whose list lacks the doc contributes its metric's missing-vector score, also when the doc has a
 * vector there.  Outputs [nq][k_out]: the top k_out by (final desc, segment asc, doc asc), the vector
 * score (sum of the clause scores found), out_count[q] = rows filled, out_total[q] = the union size.
 * alpha / boost [nq][n_clauses] (boost NULL = 1.0); q_filter[q] < 0 or a NULL array = no filter, else
 * a filter id of slg_index_add_filter*.  n_clauses outside 1..SLG_MAX_VECTOR_CLAUSES, cand_size
 * outside 1..SLG_MAX_VECTOR_CANDIDATES or k_out > SLG_MAX_K: SLG_ERR_UNSUPPORTED; a NULL or
 * inconsistent argument: SLG_ERR_INVALID, all before any device work.  The _device form takes device
 * arrays (clause_field stays on the host) and is asynchronous on the index stream; it cannot check
 * q_filter ids, and an id that names no filter registered for every segment matches nothing.
 */
int slg_vector_search_batch(slg_index *index, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                            const float *qvecs, const float *alpha, const float *boost,
                            const int32_t *q_filter, uint32_t cand_size, uint32_t k_out,
                            uint32_t *out_doc, uint32_t *out_seg, float *out_score, float *out_vec_score,
                            uint32_t *out_count, uint64_t *out_total);
int slg_vector_search_batch_device(slg_index *index, uint32_t nq, uint32_t n_clauses,
                                   const uint32_t *clause_field, const float *d_qvecs, const float *d_alpha,
                                   const float *d_boost, const int32_t *d_q_filter, uint32_t cand_size,
                                   uint32_t k_out, uint32_t *d_out_doc, uint32_t *d_out_seg, float *d_out_score,
                                   float *d_out_vec_score, uint32_t *d_out_count, uint64_t *d_out_total);

/*
 * Two-pass vector search over a reduced-precision copy of the store.
 *
 * slg_index_quantize_vector_field builds, on the device, a bf16 copy of every segment's store of vector field
 * `field` (0 = the field of the segment descriptors, else an id of slg_index_add_vector_field): each f32 value
 * rounded to nearest even (a NaN stays a NaN, +-inf stays +-inf, an f32 denormal rounds like any other value),
 * rows in the store's order and shared vec_offsets, each row padded with zeros, and beside each row its f32
 * squared norm, summed left to right over the f32 row.  The copy is part of the index state: it costs half the
 * store's bytes again, slg_index_update_deleted leaves it alone, slg_index_remove_segment drops that segment's,
 * and slg_index_add_segment quantises the new segment's field-0 store when field 0 has a copy (other fields hold
 * no vectors for a new segment).  Calling it again for the same field does nothing and returns 0; a field id that
 * does not exist: SLG_ERR_INVALID.
 *
 * slg_index_fetch_vector_copy reads a segment's copy back: up to rows_cap rows of vec_dim bf16 bit patterns each
 * (unpadded, row-major) into out_u16 and as many norms into out_norm; it returns the number of rows the copy
 * holds (0: the segment has no vectors in the field; the arrays may be NULL when rows_cap is 0), or a negative
 * error code (SLG_ERR_INVALID: the field has no copy, or no such segment).
 *
 * slg_vector_search_batch_approx[_device]: the arguments, outputs and checks of slg_vector_search_batch[_device],
 * plus refine.  Per clause, a first pass scores every doc from the bf16 copy (queries rounded to bf16, products
 * on v_mfma_f32_16x16x32_bf16 with f32 accumulation; L2 as |x|^2 + |q|^2 - 2 x.q from the f32 norms) and keeps the
 * best `refine`; a second pass scores those again from the f32 store in the exact scan's own arithmetic and keeps
 * the best cand_size; union, blend and top k_out follow as in the exact call.
 *   - Every returned score (out_score, out_vec_score) is bit for bit the exact call's score of that doc against
 *     the same clause lists; only the choice of the docs that reach the second pass is approximate.
 *   - A doc of the exact call's clause list can be missing from the list only if its exact score lies within the
 *     first pass's error of the score at the `refine` boundary (cosine of unit vectors: below 2^-7 * |boost|).
 *   - refine >= the number of live docs with a vector in the field makes the call identical to the exact one.
 * refine outside cand_size..SLG_MAX_VECTOR_CANDIDATES: SLG_ERR_UNSUPPORTED (checked first); a clause whose field
 * has no copy: SLG_ERR_INVALID, the message names the field; all before any device work.  The _device form is
 * asynchronous on the index stream and makes no host round trip between the passes.  out_total is the union size
 * of the refined cand_size lists.
 */
int slg_index_quantize_vector_field(slg_index *index, uint32_t field);
int slg_index_fetch_vector_copy(slg_index *index, uint32_t field, uint32_t seg, uint16_t *out_u16, float *out_norm,
                                uint32_t rows_cap);
int slg_vector_search_batch_approx(slg_index *index, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                                   const float *qvecs, const float *alpha, const float *boost,
                                   const int32_t *q_filter, uint32_t cand_size, uint32_t refine, uint32_t k_out,
                                   uint32_t *out_doc, uint32_t *out_seg, float *out_score, float *out_vec_score,
                                   uint32_t *out_count, uint64_t *out_total);
int slg_vector_search_batch_approx_device(slg_index *index, uint32_t nq, uint32_t n_clauses,
                                          const uint32_t *clause_field, const float *d_qvecs, const float *d_alpha,
                                          const float *d_boost, const int32_t *d_q_filter, uint32_t cand_size,
                                          uint32_t refine, uint32_t k_out, uint32_t *d_out_doc, uint32_t *d_out_seg,
                                          float *d_out_score, float *d_out_vec_score, uint32_t *d_out_count,
                                          uint64_t *d_out_total);

/*
 * Vector search over an inverted-file (IVF) index of a vector field: probe the nearest lists, exact scores.
 *
 * slg_index_cluster_vector_field groups the docs of every segment that have a vector in `field` (0 = the field of
 * the segment descriptors, else an id of slg_index_add_vector_field) into n_lists lists around the caller's
 * centroids, used as given.  A doc goes to the centroid with the greatest metric_similarity(row, centroid) in the
 * exact scan's own arithmetic (cosine: the fmaf chain with NaN -> 0; L2: -sqrt(sum (x - y)^2)); equal scores go to
 * the lowest list id; deleted docs are assigned too (tombstones apply at search time); inside a list the docs
 * ascend; an empty list is legal.  Assignment (an exact scan of the centroids with the store's rows as queries and
 * a top-1) and list build (count, exclusive scan, ordered fill) run on the device and are deterministic.  The lists
 * and the centroid tables are part of the index state: 4 bytes per doc with a vector plus the tables, no second
 * copy of the store.  slg_index_update_deleted leaves them alone, slg_index_remove_segment drops that segment's,
 * and a segment added by slg_index_add_segment is unclustered in every field.  Calling the function again builds
 * a new state: n_lists 0 leaves (or makes) a segment unclustered, SLG_KEEP_VECTOR_LISTS keeps what the segment
 * has (nothing to keep: it stays unclustered).  SLG_ERR_INVALID: no such field, n_segs other than the index's
 * segment count, n_lists > 0 with NULL centroids or on a segment without vectors in the field;
 * SLG_ERR_UNSUPPORTED: n_lists > SLG_MAX_VECTOR_LISTS; all before any device work.
 *
 * slg_index_fetch_vector_lists reads a segment's lists back: it returns n_lists (0: unclustered, or no vectors in
 * the field) or a negative code (SLG_ERR_INVALID: no such field or segment), and writes, up to the caps,
 * min(n_lists, lists_cap) + 1 entries of out_list_begin, the docs list after list into out_docs (docs_cap of them at
 * most) and min(n_lists, lists_cap) rows of the centroid table as stored into out_centroids.  The arrays may be NULL
 * when their caps are 0.
 *
 * slg_vector_search_batch_ivf[_device]: the arguments, outputs and checks of slg_vector_search_batch[_device], plus
 * nprobe.  Per query q and clause c (field f):
 *   1. the lists of all clustered segments of f form one list space ordered by (segment asc, list asc); a list's
 *      key is metric_similarity(query, centroid) * boost[q][c] in the exact scan's arithmetic, and the best
 *      min(nprobe, lists of f) by (key desc, segment asc, list asc) are probed (a negative boost probes the
 *      farthest lists, where its best docs are);
 *   2. the candidates are the docs of the probed lists and every doc of the unclustered segments of f, which are
 *      scanned whole and do not count against nprobe;
 *   3. of those, the docs that are live and pass q_filter[q] are scored as in the exact call, and the best
 *      cand_size by (score desc, segment asc, doc asc) are the clause list;
 *   4. union, blend, top k_out, out_count and out_total are the exact call's.
 * Guarantees:
 *   - every out_score / out_vec_score is bit for bit the exact call's score of that doc against the same clause
 *     lists;
 *   - with one clause the call is byte-identical to slg_vector_search_batch under a filter that is the query's
 *     filter AND "the doc is in a probed list or an unclustered segment";
 *   - nprobe >= the number of lists of every clause's field makes it byte-identical to the exact call.
 * nprobe outside 1..SLG_MAX_VECTOR_PROBES: SLG_ERR_UNSUPPORTED (checked first); cand_size > 64:
 * SLG_ERR_UNSUPPORTED (only the fused top-k form of the scan is built: use the exact or the two-pass call); a clause
 * whose field has no clustered segment: SLG_ERR_INVALID, the message names the field; all before any device work.
 * The _device form is asynchronous on the index stream and makes no host round trip between its steps.
 */
#define SLG_MAX_VECTOR_LISTS  65536u       /* lists of one segment of one field */
#define SLG_MAX_VECTOR_PROBES 256u
#define SLG_KEEP_VECTOR_LISTS 0xFFFFFFFFu  /* n_lists: leave this segment's lists as they are */
typedef struct {
  uint32_t n_lists;        /* 0: the segment is (or becomes) unclustered; SLG_KEEP_VECTOR_LISTS: unchanged */
  const float *centroids;  /* [n_lists * vec_dim] row-major host array, used as given */
} slg_vector_lists_desc;
int slg_index_cluster_vector_field(slg_index *index, uint32_t field, const slg_vector_lists_desc *per_segment,
                                   uint32_t n_segs);
int slg_index_fetch_vector_lists(slg_index *index, uint32_t field, uint32_t seg, uint32_t *out_list_begin,
                                 uint32_t *out_docs, float *out_centroids, uint32_t lists_cap, uint32_t docs_cap);
int slg_vector_search_batch_ivf(slg_index *index, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                                const float *qvecs, const float *alpha, const float *boost, const int32_t *q_filter,
                                uint32_t cand_size, uint32_t nprobe, uint32_t k_out, uint32_t *out_doc,
                                uint32_t *out_seg, float *out_score, float *out_vec_score, uint32_t *out_count,
                                uint64_t *out_total);
int slg_vector_search_batch_ivf_device(slg_index *index, uint32_t nq, uint32_t n_clauses,
                                       const uint32_t *clause_field, const float *d_qvecs, const float *d_alpha,
                                       const float *d_boost, const int32_t *d_q_filter, uint32_t cand_size,
                                       uint32_t nprobe, uint32_t k_out, uint32_t *d_out_doc, uint32_t *d_out_seg,
                                       float *d_out_score, float *d_out_vec_score, uint32_t *d_out_count,
                                       uint64_t *d_out_total);

/*
 * Training the centroids of an IVF index on the device: Lloyd steps over the f32 store.
 *
 * slg_index_train_vector_field computes, for every segment s with per_segment[s].n_lists in
 * 1..SLG_MAX_VECTOR_LISTS, centroids on the device from the segment's own store and builds the segment's lists
 * around them in a new index state.  The lifecycle is slg_index_cluster_vector_field's: n_lists 0 leaves (or makes)
 * the segment unclustered, SLG_KEEP_VECTOR_LISTS keeps the segment's list object by reference, earlier states keep
 * theirs, and slg_index_fetch_vector_lists returns the trained centroids.  The algorithm, in the order of its
 * floating-point operations (R = the rows of the segment's value array, dim = the field's dimension):
 *   start   C_0 = init when it is given, used as given.  Otherwise centroid i is row floor(i * R / n_lists) of the
 *           value array (u64 arithmetic), copied on the device as stored.
 *   assign  A_t = assign(C_{t-1}), t = 1 .. iters, is the assignment of slg_index_cluster_vector_field for those
 *           centroids: the exact scan's arithmetic, ties to the lowest list, deleted docs assigned (and summed:
 *           tombstones apply at search time only), docs without a vector in no list, docs ascending in a list.
 *   stop    moved_t = the rows (of the value array) whose list differs from the one in A_{t-1}; moved_1 = R.  If
 *           t > 1 and moved_t == 0, training stops with C_{t-1}.  That is a fixed point, because the update depends
 *           only on the assignment and an empty list keeps its centroid: the early stop never changes the result.
 *   update  C_t = update(A_t, C_{t-1}), per list l with its n docs ascending:
 *             sum[d]: the docs are cut into consecutive chunks of SLG_VECTOR_TRAIN_CHUNK; per chunk an f64 sum of
 *               (double)row[d] in doc order from +0.0; the chunk sums added in chunk order from +0.0;
 *             m[d] = (float)(sum[d] / (double)n);
 *             s = sum over d ascending of (double)m[d] * (double)m[d], from +0.0;
 *             the list adopts a new centroid iff n > 0, s is finite and (cosine only) s > 0; otherwise
 *               C_t[l] = C_{t-1}[l] bit for bit;
 *             the new centroid is m (L2) or (float)((double)m[d] / sqrt(s)) (cosine).
 *           Division, square root and the f64 -> f32 conversions are IEEE round-to-nearest-even, correctly rounded;
 *           nothing is contracted.  No floating-point atomics: the bytes do not depend on the device's schedule.
 *   finish  the state's lists are assign(final centroids): A_t after an early stop, one more assignment after the
 *           last step, assign(C_0) with iters 0.
 * Guarantee: the resulting state is byte-identical to slg_index_cluster_vector_field called with the centroids
 * slg_index_fetch_vector_lists returns.
 * out_stats (NULL, or [n_segs]), per trained segment: iters_run = the updates applied; moved = moved_t of the last
 * assignment made by a step t <= iters (0 after an early stop; 0 with iters 0: the finishing assignment is not a
 * step); empty_lists and max_len of the final lists.  Untrained segments get zeros.  Nothing is written on error.
 * Errors, all before any device work: SLG_ERR_UNSUPPORTED: iters > SLG_MAX_VECTOR_TRAIN_ITERS on a trained segment
 * (checked first, before the index is looked at), n_lists > SLG_MAX_VECTOR_LISTS; SLG_ERR_INVALID: NULL index, no
 * such field, n_segs other than the index's segment count, n_lists > 0 on a segment without vectors in the field,
 * init NULL with n_lists greater than R.
 * The loop runs on the index stream with scratch released before the call returns (two list ids per row, the
 * partial sums: 8 bytes x dim per (list, chunk)); per step the host reads back moved and the list lengths.
 * Not built: training on a sample; k-means++ or seeded starts on the device (pass init); re-seeding of empty
 * lists; training across segments; training over the bf16 copy.
 */
#define SLG_MAX_VECTOR_TRAIN_ITERS 256u
#define SLG_VECTOR_TRAIN_CHUNK     256u   /* docs of one partial sum, see "update" */
typedef struct {
  uint32_t n_lists;     /* 0: the segment is (or becomes) unclustered; SLG_KEEP_VECTOR_LISTS: unchanged; else train */
  uint32_t iters;       /* Lloyd steps at most, 0 .. SLG_MAX_VECTOR_TRAIN_ITERS */
  const float *init;    /* [n_lists * vec_dim] host array, used as given; NULL: rows of the store, see "start" */
} slg_vector_train_desc;                 /* 16 bytes */
typedef struct { uint32_t iters_run, moved, empty_lists, max_len; } slg_vector_train_stats;
int slg_index_train_vector_field(slg_index *index, uint32_t field, const slg_vector_train_desc *per_segment,
                                 uint32_t n_segs, slg_vector_train_stats *out_stats /* [n_segs] or NULL */);

/*
 * Hybrid text + vector search: one request with a text query and vector clauses (api/reader.rs:2754-2775:
 * collect_vector_maps with require_text_match = true, then merge_vector_hits, :2474-2537).  Per query:
 *   1. the matched set M = every doc the text query matches that is not deleted and passes q_filter (and
 *      minimum_should_match, where the batch shape supports it);
 *   2. the BM25 hits = the top k of M by (score desc, segment asc, doc asc): the batch's own rows, bit for bit
 *      those of slg_batch_prepare_plans for the same queries at the same k;
 *   3. per clause c (field clause_field[c], as in slg_vector_search_batch) every doc of M with a vector in the
 *      field scores metric_similarity * boost[q][c]; the best cand_size by (score desc, segment asc, doc asc)
 *      form the clause's list.  Exact where the reference searches an HNSW graph, every predicate applied
 *      before the truncation: recall is never below the reference's;
 *   4. union = BM25 hits + all clause lists; a union doc's bm25 is its score among the BM25 hits, else 0.0
 *      (:2496-2500, also though it matches the text); each clause blends as compute_hybrid_score (:225-254),
 *      a clause whose list lacks the doc with its metric's missing-vector score; final = sum / n_clauses; when
 *      every alpha <= 0 a union doc found in no clause list is dropped (:2494,2504);
 *   5. rows [nq][k_out] = the top by (final desc under f32::total_cmp, segment asc, doc asc); out_vec_score =
 *      the sum of the clause scores found, and for a row no clause list holds (the reference's None) the
 *      missing-vector score of clause 0's metric (-1.0 / f32::MIN), as slg_rerank_fields_batch writes it;
 *      out_count[q] = rows filled, out_total[q] = the union size after the drop.
 *
 * slg_batch_prepare_hybrid plans the text side as slg_batch_prepare_sorted does (every matched doc becomes a
 * candidate with its exact score: no threshold seed, no MaxScore) and accepts every query shape that call
 * accepts; slg_batch_run leaves the BM25 top k in the batch's rows (slg_batch_fetch, slg_batch_device_results)
 * and keeps the candidates.  slg_batch_hybrid_device then runs steps 3-5 asynchronously on the batch's stream
 * (no host round trip after slg_batch_run; device arrays, clause_field on the host; qvecs / alpha / boost as in
 * slg_vector_search_batch).  It may be called again on the same batch with other clauses.  The gathered keys
 * take 8 bytes x matched docs x clauses; the queries of a batch are processed in ranges whose keys fit a
 * quarter of the buffer pool's cap (at most 1 GiB), and a single query that does not fit fails with
 * SLG_ERR_OOM: never a partial result.  slg_search_batch_hybrid is the one-call form with host arrays.
 * k = 0 is allowed: there are no BM25 hits, the union is the clause lists alone and every bm25 is 0.0 (no
 * select kernel runs; the gather drops deleted and filtered docs itself, by the same bitmaps).
 *
 * n_clauses outside 1..SLG_MAX_VECTOR_CLAUSES, cand_size outside 1..SLG_MAX_VECTOR_CANDIDATES, k or k_out above
 * SLG_MAX_K, or clause vectors of more than 36 Ki floats per query: SLG_ERR_UNSUPPORTED; a NULL or inconsistent
 * argument, a batch that has not run or was not made by slg_batch_prepare_hybrid: SLG_ERR_INVALID; all before
 * any device work.  slg_batch_run_sharded*, slg_batch_fetch_sharded, slg_batch_matched_counts and
 * slg_batch_cursor_seen refuse a hybrid batch with SLG_ERR_UNSUPPORTED; the coalescer builds its own batches
 * and has no hybrid request kind.
 */
slg_batch *slg_batch_prepare_hybrid(slg_index *index, uint32_t nq, const uint32_t *q_offsets,
                                    const uint32_t *q_term_ids, const float *q_weights,
                                    const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                                    uint32_t k, int strategy);
int slg_batch_hybrid_device(slg_batch *batch, uint32_t n_clauses, const uint32_t *clause_field,
                            const float *d_qvecs, const float *d_alpha, const float *d_boost, uint32_t cand_size,
                            uint32_t k_out, uint32_t *d_out_doc, uint32_t *d_out_seg, float *d_out_score,
                            float *d_out_vec_score, uint32_t *d_out_count, uint64_t *d_out_total);
int slg_search_batch_hybrid(slg_index *index, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                            const float *q_weights, const slg_score_plans *plans_or_null,
                            const int32_t *q_filter_or_null, uint32_t k, int strategy, uint32_t n_clauses,
                            const uint32_t *clause_field, const float *qvecs, const float *alpha,
                            const float *boost, uint32_t cand_size, uint32_t k_out, uint32_t *out_doc,
                            uint32_t *out_seg, float *out_score, float *out_vec_score, uint32_t *out_count,
                            uint64_t *out_total);

/*
 * Query rescore: SearchRequest::rescore { window_size, query, score_mode } (api/types.rs:523-545), carried out by
 * rescore_hits (api/reader.rs:3238-3398) and combine_rescore_scores (:3623-3629).  Per query, after the first
 * pass has left its rows (count <= k, by score desc, segment asc, doc asc):
 *   1. w = min(q_window[q], count).  w == 0, or a rescore query without a term: the rows stay as they are.
 *   2. A row (segment s, doc d, score o) of the first w is MATCHED if at least max(q_min_match[q], 1) leaves of
 *      the rescore query have a term whose list in segment s holds d.  A row that is not matched keeps its
 *      score untouched: it is neither multiplied by 0 nor removed (:3319-3321).
 *   3. For a matched row every rescore term t whose list in segment s holds d adds impact * weight_t to its
 *      leaf (impact = the BM25 score of the posting at weight 1, score_tf's base; one f32 product, one f32
 *      add, never fused), the terms of a leaf IN QUERY-TERM ORDER; the leaves are combined as the first pass
 *      combines a flat plan (slg_batch_prepare_plan): SLG_PLAN_SUM, or SLG_PLAN_DISMAX with a tie breaker in
 *      [0, 1], leaves in leaf order, a DisMax leaf without a posting counting as 0.0.  That is the rescore
 *      score r.  (The reference accumulates a row's term scores by walking a HashMap, :3290-3300, so its own
 *      summation order is not defined; this library fixes it, as its first pass does.)
 *   4. new score = o + r (SLG_RESCORE_TOTAL, _SUM), o * r (_MULTIPLY), max(o, r) (_MAX), min(o, r) (_MIN; max
 *      and min as f32::max / f32::min: a NaN operand yields the other one): plain f32 operations.
 *   5. The first w rows are sorted again by (score desc under f32::total_cmp, segment asc, doc asc).  Rows
 *      from w on keep their place and score, also where a window row now scores below them: the reference
 *      sorts hits[..window] only (:3393-3396).  out_count does not change.
 * The rescore applies no tombstone or filter test of its own: first-pass rows are live and filtered.
 *
 * The rescore queries come in the CSR form of the first pass (q_offsets [nq + 1], q_term_ids [total x n_segs],
 * q_weights [total]) with the flat plan arrays of slg_batch_prepare_plan (each may be NULL, same defaults),
 * q_min_match [nq] or NULL, q_window [nq], and q_mode [nq] or NULL (total).  Rescore queries whose score tree
 * has more than one level of Sum / DisMax over the leaves, function scores and phrases (a rescore query takes no
 * phrase spec; phrases of the first pass: slg_batch_prepare_phrase) are not accepted by this form: the caller
 * keeps such requests on the CPU scorer.
 *
 * slg_batch_prepare_rescore is slg_batch_prepare_plans plus the spec; the batch goes through slg_batch_run /
 * _fetch / _device_results / _set_stream as any batch.  slg_batch_run enqueues the rescore kernel behind the
 * first pass on the batch's stream, so several batches stay in flight and the rows a caller sees are the
 * rescored ones; running a batch again scores from scratch.  The rescore terms are resolved against the index
 * state the batch was prepared on.  slg_batch_fetch_rescore waits for the batch and copies [nq * k] arrays
 * parallel to the rows (each may be NULL): the first-pass score, r (0.0 where the row was not rescored), and
 * 1 where the row was rescored.  slg_search_batch_rescore is the one-call form with host arrays.
 *
 * Before any device work: a NULL spec, inconsistent offsets, a mode or plan out of range, a tie outside [0, 1]
 * or not finite, a weight that is not finite, a term id out of range, or more than SLG_MAX_QUERY_TERMS rescore
 * terms in a query: SLG_ERR_INVALID.  A window that, capped at k (a window never reaches past the k rows), is
 * above SLG_MAX_RESCORE_WINDOW (= SLG_MAX_RERANK_K, the widest register top-k the library has), or a rescore
 * query whose terms x segments exceed 2048 table entries: SLG_ERR_UNSUPPORTED (CPU scorer).  slg_batch_fetch_rescore on a batch without rescore, or one that has not
 * run: SLG_ERR_INVALID.  slg_batch_run_sharded* and slg_batch_fetch_sharded refuse a rescore batch with
 * SLG_ERR_UNSUPPORTED.  Not built: rescore on sorted, cursor, hybrid, vector-only and aggregation batches,
 * and in the coalescer (none of their prepare calls takes a rescore spec; behind a clause stage:
 * slg_batch_prepare_request, "compound requests" below).
 */
enum { SLG_RESCORE_TOTAL = 0, SLG_RESCORE_MULTIPLY = 1, SLG_RESCORE_SUM = 2, SLG_RESCORE_MAX = 3, SLG_RESCORE_MIN = 4 };
#define SLG_MAX_RESCORE_WINDOW 1024u
typedef struct slg_rescore_spec {
  const uint32_t *q_offsets;   /* [nq + 1] rescore terms of every query */
  const uint32_t *q_term_ids;  /* [total x n_segs] per-segment term ids, SLG_NO_TERM where absent */
  const float *q_weights;      /* [total] */
  const uint32_t *q_leaf;      /* [total] leaf of every rescore term; NULL: term i of a query is leaf i */
  const int32_t *q_plan;       /* [nq] SLG_PLAN_SUM | SLG_PLAN_DISMAX over the leaves; NULL: Sum */
  const float *q_tie;          /* [nq] DisMax tie breaker in [0, 1]; NULL: 0 */
  const uint32_t *q_nleaves;   /* [nq] leaves of the plan; NULL: 1 + the largest leaf named */
  const uint32_t *q_min_match; /* [nq] leaves that must hold a row's doc; NULL, 0 and 1: any */
  const uint32_t *q_window;    /* [nq] window_size; min(window, k) <= SLG_MAX_RESCORE_WINDOW */
  const int32_t *q_mode;       /* [nq] SLG_RESCORE_*; NULL: total */
} slg_rescore_spec;
slg_batch *slg_batch_prepare_rescore(slg_index *index, uint32_t nq, const uint32_t *q_offsets,
                                     const uint32_t *q_term_ids, const float *q_weights,
                                     const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                                     const slg_rescore_spec *rescore, uint32_t k, int strategy);
int slg_batch_fetch_rescore(slg_batch *batch, float *out_first_score, float *out_rescore_score,
                            uint32_t *out_rescored);
int slg_search_batch_rescore(slg_index *index, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                             const float *q_weights, const slg_score_plans *plans_or_null,
                             const int32_t *q_filter_or_null, const slg_rescore_spec *rescore, uint32_t k,
                             int strategy, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                             uint32_t *out_count, float *out_first_score, float *out_rescore_score,
                             uint32_t *out_rescored);

/* ---------------------------------------------------------------------------------------------------------
 * Boolean queries: `bool { must, should, must_not, minimum_should_match }` over term clauses and the query
 * string's `+a -b` form.  The reference walks the union of the scored lists and asks accept(doc) for each doc;
 * accept evaluates QueryEvaluator::matches_node (api/reader.rs:1485-1565), whose term-group test is a binary
 * search of the doc in the group's posting lists (term_group_matches, :1571-1580).  Here, in flat form:
 *
 * A query has a clause table of GROUPS.  A group is one or more terms (one query word over its fields) and
 * HOLDS a doc of segment s if any of its terms has a posting of the doc in s.  Every group has a kind
 * (SLG_BOOL_MUST / _SHOULD / _MUST_NOT) and the query a q_min_should.  A candidate — a doc of a scored list —
 * is accepted iff every MUST group holds it, no MUST_NOT group holds it, and at least q_min_should SHOULD groups
 * hold it (0: no should requirement; more than the query has SHOULD groups: nothing matches).  Tombstones and
 * q_filter apply as in every batch.  `Bool` with Term children (:1527-1563): the caller passes the reference's
 * minimum_should_match, its default rule (:1553-1561) applied.  A query string (:1490-1518): term groups are
 * SHOULD groups with q_min_should = minimum_should_match.unwrap_or(1), not-terms are MUST_NOT groups.
 *
 * Clause terms are independent of the scored terms (a must / should term is normally scored too, a must_not
 * term never is).  Only docs of the scored lists are candidates, as in the reference: a query whose scored
 * lists are all empty returns nothing.  A clause term that is SLG_NO_TERM in a segment has no posting there: a
 * MUST group whose terms are all absent from a segment rejects every candidate of that segment, an absent
 * MUST_NOT term rejects nothing.  A query without a group is untouched (its q_min_should is not looked at);
 * queries with and without groups mix in one batch.
 *
 * Scores are untouched: an accepted doc has the exact score of the first pass, under any score plan.  The
 * plans' q_min_match must be NULL, 0 or 1 (SLG_ERR_INVALID otherwise): the clause table is the one place that
 * states it — which also lifts its limits (more than 8 scored lists, nested plans).
 *
 * The clause terms of query q are rows c_offsets[q] .. c_offsets[q + 1] - 1 of c_term_ids (one id per segment,
 * as q_term_ids) and c_group; c_group[i] is the term's group inside its query: non-decreasing from 0 without
 * gaps, so every group g_offsets[q] .. g_offsets[q + 1] - 1 of g_kind has a term.
 *
 * slg_batch_prepare_bool is slg_batch_prepare_plans (sort NULL: score order) or slg_batch_prepare_sorted (a field
 * sort) plus the spec.  The batch is planned as a sorted batch is — every doc of the scored lists is scored,
 * no threshold seed, no MaxScore — and slg_batch_run enqueues one kernel between the scoring kernel and the
 * select that drops the candidates the clause table rejects.  slg_batch_run / _fetch / _device_results / _sync /
 * _set_stream as for any batch; slg_batch_matched_counts for the sorted form: it counts accepted docs.
 * slg_stats.scored_docs = the count of a batch without clauses (see slg_stats) minus the docs the clause table
 * rejected.  The clause terms are resolved against the index state the batch was prepared on.
 * slg_search_batch_bool is the one-call form with host arrays; stats may be NULL; out_matched may be NULL and
 * must be NULL without a sort spec.
 *
 * Errors, all before any device work.  SLG_ERR_INVALID: a NULL spec or array, offsets that decrease, a c_group
 * that decreases, skips a number or names a group the query does not have, a group without a term, an unknown
 * kind, a term id out of range, q_min_match > 1 in the plans.  SLG_ERR_UNSUPPORTED (CPU scorer): more than
 * SLG_MAX_BOOL_GROUPS groups or SLG_MAX_BOOL_TERMS clause terms in a query.  slg_batch_run_sharded* and
 * slg_batch_fetch_sharded refuse a bool batch with SLG_ERR_UNSUPPORTED.  Nested matchers (a bool, dis_max or
 * query string as a child of bool) and a bool's own filter list: slg_batch_prepare_bool_tree below.  Not built
 * (CPU scorer): clause tables on hybrid, sharded and coalesced batches (with a cursor, a score stage,
 * aggregations, rescore or collapse: slg_batch_prepare_request, "compound requests" below).  Phrase children of a bool and the query string's quoted phrases:
 * slg_batch_prepare_phrase below.
 * --------------------------------------------------------------------------------------------------------- */
#define SLG_BOOL_MUST 0
#define SLG_BOOL_SHOULD 1
#define SLG_BOOL_MUST_NOT 2
#define SLG_MAX_BOOL_GROUPS 32u   /* groups of one query (one bit each in the kernel's masks) */
#define SLG_MAX_BOOL_TERMS 64u    /* clause terms of one query */
typedef struct slg_bool_spec {
  const uint32_t *c_offsets;    /* [nq + 1] into c_term_ids rows / c_group */
  const uint32_t *c_term_ids;   /* [n_clause_terms x n_segs], rows as q_term_ids, SLG_NO_TERM where absent */
  const uint32_t *c_group;      /* [n_clause_terms] group of the term inside its query, non-decreasing, from 0, no gaps */
  const uint32_t *g_offsets;    /* [nq + 1] into g_kind */
  const int32_t *g_kind;        /* [n_groups] SLG_BOOL_* */
  const uint32_t *q_min_should; /* [nq] or NULL (= 0) */
} slg_bool_spec;
slg_batch *slg_batch_prepare_bool(slg_index *index, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                                  const float *q_weights, const slg_score_plans *plans_or_null,
                                  const int32_t *q_filter_or_null, const slg_sort_spec *sort_or_null,
                                  const slg_bool_spec *spec, uint32_t k, int strategy);
int slg_search_batch_bool(slg_index *index, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                          const float *q_weights, const slg_score_plans *plans_or_null,
                          const int32_t *q_filter_or_null, const slg_sort_spec *sort_or_null,
                          const slg_bool_spec *spec, uint32_t k, int strategy, uint32_t *out_doc, uint32_t *out_seg,
                          float *out_score, uint32_t *out_count, slg_stats *stats_or_null,
                          uint64_t *out_matched_or_null);

/* ---------------------------------------------------------------------------------------------------------
 * Nested boolean matchers: the matcher TREE of QueryEvaluator::matches_node (api/reader.rs:1485-1565), in which
 * a `Bool` may hold `Bool`, `DisMax`, `QueryString` and `MatchAll` children and carries a `filter` list of its
 * own — `bool{must:[..], should:[bool{..}, dis_max{..}]}`, a multi_match under a must, a negated sub-query.
 *
 * A query's matcher is a table of LEAVES and a table of NODES.
 *
 * Leaves.  A TERM GROUP is one or more clause terms and HOLDS a doc of segment s iff one of its terms has a
 * posting of the doc in s (the bool batch's rule, term_group_matches); a term that is SLG_NO_TERM in a segment, or
 * has df 0 there, has no posting there.  A FILTER LEAF is a registered filter id (slg_index_add_filter*,
 * slg_index_add_filter_trees) and holds the doc iff the doc passes that filter in its segment; a segment
 * given no mask when the filter was registered passes every live doc, and a filter that predates a segment
 * (slg_index_add_segment) is refused here as it is in q_filter: SLG_ERR_INVALID, "unknown filter id", until it is
 * registered again.  A registered bitmap carries its segment's tombstones, so a tombstoned doc passes no filter
 * leaf: no row changes (tombstones apply on top anyway), only slg_stats.scored_docs sees it.  A query's leaves are
 * numbered term groups first, filter leaves behind them.
 *
 * Nodes.  A node is a list of (child, kind) pairs, kind SLG_BOOL_MUST / _SHOULD / _MUST_NOT, and a min_should.
 * Its value is
 *     every MUST child true  &&  no MUST_NOT child true  &&  count(true SHOULD children) >= min_should.
 * A child is a leaf or an EARLIER node: the node table is in post-order, a child's index is below its parent's,
 * the last node is the root, and the root's value is the candidate's verdict.  Tombstones and q_filter apply on
 * top, as in every batch.
 *
 * Every node kind of the reference folds into this form (the caller folds; searchlite_amd/booltree.py does it):
 *   Bool         its must / should / must_not children with their kinds, its `filter` list as MUST filter leaves,
 *                min_should = minimum_should_match with the default rule (:1553-1561) applied: 0 without should
 *                children, 1 when must and filter are both empty, else 0.
 *   DisMax       all children SHOULD, min_should 1 (an empty DisMax: no children, min_should 1 — never true).
 *   QueryString  not-groups MUST_NOT, term groups SHOULD, min_should = minimum_should_match.unwrap_or(1) when it
 *                has term groups, else 0; no groups at all: no children, min_should 1 — never true (:1491-1496).
 *   MatchAll     no children, min_should 0.
 *   a matcher that is one Term: one node with that leaf as a MUST child.
 *   Phrase leaves are not built in a tree: the caller refuses them (SLG_ERR_UNSUPPORTED).
 *
 * Everything else is the bool batch's, unchanged.  Clause terms are independent of the scored terms; only docs of
 * the scored lists are candidates; an accepted doc has the exact score of the first pass, bit for bit, under any
 * score plan and either scoring kernel; a query without a node is left as it is, and such queries mix with others
 * in a batch; slg_stats.scored_docs = the count of the batch without a matcher minus the docs the matcher
 * rejected; a sorted batch's matched counts see survivors only; the plans' q_min_match must be NULL, 0 or 1; the
 * batch is planned as a bool batch is (candidates mode, no threshold seed, no MaxScore); clause terms and filter
 * ids are resolved against the index state the batch was prepared on.
 *
 * The spec.  Term groups: c_offsets / c_term_ids / c_group / g_offsets as in slg_bool_spec, without kinds
 * (g_offsets[q + 1] - g_offsets[q] = the query's term groups).  Filter leaves: f_filter[f_offsets[q] ..
 * f_offsets[q + 1]).  Nodes: node j of query q is entry n = n_offsets[q] + j of n_min_should, its children
 * e_child / e_kind [e_offsets[n] .. e_offsets[n + 1]).  A child index below the query's leaf count names a leaf;
 * otherwise it is leaf count + the index of an earlier node of the same query.
 *
 * slg_batch_prepare_bool_tree / slg_search_batch_bool_tree have the argument shape and the life cycle of the two
 * bool calls.  slg_batch_run enqueues ONE kernel between the scoring kernel and the select; a batch without
 * slices, or whose queries have no node, launches nothing.  One candidate's state is a 64-bit mask — bits 0-31
 * the leaves, bits 32-63 the nodes — hence the limits.
 *
 * Errors, all before any device work.  SLG_ERR_INVALID: a NULL spec or array, offsets that decrease, a c_group
 * that decreases, skips a number or names a group the query does not have, a group without a term, an unknown
 * kind, a child index that is not below its node, a leaf — or a node other than the root — that no node
 * references, a query with leaves but no node, a term id out of range, an unknown filter id, q_min_match > 1 in
 * the plans.  SLG_ERR_UNSUPPORTED (CPU scorer): more than SLG_MAX_BOOL_TREE_LEAVES leaves, SLG_MAX_BOOL_TREE_NODES
 * nodes or SLG_MAX_BOOL_TERMS clause terms in a query; the same child twice in one node (the reference would
 * count it twice, a mask cannot).  slg_batch_run_sharded* and slg_batch_fetch_sharded refuse the batch with
 * SLG_ERR_UNSUPPORTED.  Not built (CPU scorer): phrase leaves in a tree, and trees on hybrid,
 * sharded and coalesced batches (with a cursor, a score stage, aggregations, rescore or collapse:
 * slg_batch_prepare_request, "compound requests" below).
 * --------------------------------------------------------------------------------------------------------- */
#define SLG_MAX_BOOL_TREE_LEAVES 32u  /* term groups + filter leaves of one query (bits 0-31 of the kernel's masks) */
#define SLG_MAX_BOOL_TREE_NODES 32u   /* nodes of one query (bits 32-63) */
typedef struct slg_bool_tree_spec {
  const uint32_t *c_offsets;    /* [nq + 1] into c_term_ids rows / c_group */
  const uint32_t *c_term_ids;   /* [n_clause_terms x n_segs], rows as q_term_ids, SLG_NO_TERM where absent */
  const uint32_t *c_group;      /* [n_clause_terms] term group of the term inside its query, non-decreasing, from 0, no gaps */
  const uint32_t *g_offsets;    /* [nq + 1]: query q has g_offsets[q + 1] - g_offsets[q] term groups */
  const uint32_t *f_offsets;    /* [nq + 1] into f_filter */
  const int32_t *f_filter;      /* [n_filter_leaves] filter ids */
  const uint32_t *n_offsets;    /* [nq + 1] into n_min_should / e_offsets */
  const uint32_t *n_min_should; /* [n_nodes] */
  const uint32_t *e_offsets;    /* [n_nodes + 1] into e_child / e_kind */
  const uint32_t *e_child;      /* [n_edges] a leaf, or leaf count + an earlier node of the query */
  const int32_t *e_kind;        /* [n_edges] SLG_BOOL_* */
} slg_bool_tree_spec;
slg_batch *slg_batch_prepare_bool_tree(slg_index *index, uint32_t nq, const uint32_t *q_offsets,
                                       const uint32_t *q_term_ids, const float *q_weights,
                                       const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                                       const slg_sort_spec *sort_or_null, const slg_bool_tree_spec *spec, uint32_t k,
                                       int strategy);
int slg_search_batch_bool_tree(slg_index *index, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                               const float *q_weights, const slg_score_plans *plans_or_null,
                               const int32_t *q_filter_or_null, const slg_sort_spec *sort_or_null,
                               const slg_bool_tree_spec *spec, uint32_t k, int strategy, uint32_t *out_doc,
                               uint32_t *out_seg, float *out_score, uint32_t *out_count, slg_stats *stats_or_null,
                               uint64_t *out_matched_or_null);

/* ---------------------------------------------------------------------------------------------------------
 * Phrase queries: `"olive oil" pasta`, match_phrase with a slop, and Phrase children of a bool.  The reference
 * treats a phrase as a pure filter: QueryNode::Phrase scores nothing (query/planner.rs:622-635) and a query
 * string's phrase_groups are required, unscored groups (api/reader.rs:1502-1506).  So a phrase batch is a bool
 * batch (above) whose clause table has one more kind of group.
 *
 * POSITIONS.  slg_index_set_positions attaches the positions of segment seg's postings: pos_offsets is
 * uint64_t[P + 1] over the segment's P postings in the order of doc_ids / tfs (unpadded), positions is
 * uint32_t[pos_offsets[P]]; posting i has positions[pos_offsets[i] .. pos_offsets[i + 1]).  Host arrays are
 * borrowed for the call only.  The call builds the next index state, as every update call does; batches already
 * prepared keep the state — and the positions — they were prepared on.  slg_index_update_deleted keeps a
 * segment's positions, slg_index_remove_segment drops that segment's, slg_index_add_segment gives the new
 * segment none, and NULL, NULL removes them.  A segment without positions behaves as the reference's
 * keep_positions = false: every posting has an empty position list, so no phrase holds any doc there (not an
 * error).  Checked on the host before any device work.  SLG_ERR_INVALID: no such segment, one array NULL and
 * the other not, pos_offsets[0] != 0, offsets that decrease, positions that decrease inside a posting, a
 * position >= 2^31 (the reference does its gap arithmetic in i32).  SLG_ERR_UNSUPPORTED: more than 2^32 - 1
 * positions in the segment (told from the offsets, before a position is read).
 *
 * PHRASE GROUPS AND VARIANTS (build_phrase_runtimes, phrase_matches, api/reader.rs:1584-1720).  A phrase group
 * has a slop and zero or more VARIANTS, one per field the phrase is looked up in.  A variant is an ordered row
 * of n >= 1 terms, one per phrase position.  (More than one alternative term per position — synonym analyzers —
 * is not built: the caller keeps such requests on the CPU.)  In segment s a variant is DROPPED if any of its
 * terms is SLG_NO_TERM there or has df 0.  A group holds a doc iff any surviving variant matches it; a group
 * with no surviving variant holds nothing.
 *
 * matches_phrase (query/phrase.rs:4-48).  Every term of the variant must have a posting of the doc, and that
 * posting must have at least one position: a posting with an empty position list fails the variant, also for
 * n = 1.  For n = 1 that is all.  For n >= 2 the variant matches iff positions p0 < p1 < ... < p(n-1) exist,
 * p_i taken from term i's position list of the doc, with sum(p_i - p_(i-1) - 1) <= slop.  The sum telescopes:
 * p(n-1) - p0 <= slop + n - 1 over strictly increasing chains.  The same list may appear twice ("a a");
 * strictness then demands two different positions.  Positions of one posting are non-decreasing.
 *
 * WHERE THE GROUP GOES.  Into the clause table of a bool batch, with the same three kinds and the same formula:
 * a candidate — a doc of a scored list — is accepted iff every MUST group (term or phrase) holds it, no
 * MUST_NOT group holds it, and at least q_min_should SHOULD groups (term or phrase) hold it.  A query string
 * (reader.rs:1490-1518): phrases are MUST phrase groups, words are SHOULD term groups with q_min_should =
 * minimum_should_match.unwrap_or(1), not-terms are MUST_NOT term groups.  Bool with Term / Phrase children
 * (:1527-1563): as a bool batch, plus phrase groups of the child's kind.  Only docs of the scored lists are
 * candidates: a request without scored terms stays on the CPU.  Scores are the first pass's, bit for bit.  A
 * query without any group is untouched; such queries mix with others in a batch.
 *
 * THE SPEC is CSR, three levels deep.  The phrases of query q are p_offsets[q] .. p_offsets[q + 1] - 1 of p_kind
 * (SLG_BOOL_*) and p_slop; the variants of phrase p are v_offsets[p] .. v_offsets[p + 1] - 1; the terms of
 * variant v are rows t_offsets[v] .. t_offsets[v + 1] - 1 of t_term_ids (one id per segment, as q_term_ids), in
 * phrase order.  The term groups come in the bool spec, or bool_or_null is NULL: none.  In a query's clause
 * table the phrase groups are numbered after its term groups; term groups plus phrase groups <=
 * SLG_MAX_BOOL_GROUPS.  q_min_should [nq] or NULL (= 0) counts over both; when both specs are given the bool
 * spec's q_min_should must be NULL — one place states it, as with q_min_match, which must be NULL, 0 or 1.
 *
 * slg_batch_prepare_phrase is slg_batch_prepare_bool with the phrase spec: planned exactly as a bool batch,
 * run / fetch / matched counts / set_stream as one, the stats contract (scored_docs counts accepted docs) is
 * the bool batch's.  slg_batch_run enqueues ONE kernel between the scoring kernel and the select; it evaluates
 * the whole table, term groups and phrase groups.  Terms and positions are resolved against the index state
 * the batch was prepared on.  slg_search_batch_phrase is the one-call form.
 *
 * Errors, all before an index state is looked at.  SLG_ERR_INVALID: a NULL phrase spec or array, whatever a
 * bool batch refuses in the bool spec, a q_min_should in the bool spec, offsets that decrease, a variant
 * without a term, an unknown kind, a term id out of range, q_min_match > 1.  SLG_ERR_UNSUPPORTED (CPU scorer):
 * more than SLG_MAX_PHRASE_TERMS terms in a variant, SLG_MAX_PHRASE_VARIANTS variants in a phrase,
 * SLG_MAX_PHRASE_QUERY_TERMS variant terms in a query, a slop above SLG_MAX_PHRASE_SLOP, too many groups.
 * slg_batch_run_sharded* and slg_batch_fetch_sharded refuse a phrase batch with SLG_ERR_UNSUPPORTED.  Not built
 * (CPU scorer): phrases in rescore queries, position alternatives, nested matchers, and phrase batches on
 * hybrid, sharded and coalesced paths (with a cursor, a score stage, aggregations, rescore or collapse:
 * slg_batch_prepare_request, "compound requests" below).
 * --------------------------------------------------------------------------------------------------------- */
int slg_index_set_positions(slg_index *index, uint32_t seg, const uint64_t *pos_offsets, const uint32_t *positions);

#define SLG_MAX_PHRASE_TERMS 8u         /* terms of one variant */
#define SLG_MAX_PHRASE_VARIANTS 8u      /* variants of one phrase */
#define SLG_MAX_PHRASE_QUERY_TERMS 64u  /* variant terms of one query */
#define SLG_MAX_PHRASE_SLOP (2147483647u - 8u)
typedef struct slg_phrase_spec {
  const uint32_t *p_offsets;    /* [nq + 1] into p_kind / p_slop */
  const int32_t *p_kind;        /* [n_phrases] SLG_BOOL_* */
  const uint32_t *p_slop;       /* [n_phrases] */
  const uint32_t *v_offsets;    /* [n_phrases + 1] into the variants */
  const uint32_t *t_offsets;    /* [n_variants + 1] into the rows of t_term_ids */
  const uint32_t *t_term_ids;   /* [n_variant_terms x n_segs], rows as q_term_ids, SLG_NO_TERM where absent */
  const uint32_t *q_min_should; /* [nq] or NULL (= 0), over term and phrase SHOULD groups */
} slg_phrase_spec;
slg_batch *slg_batch_prepare_phrase(slg_index *index, uint32_t nq, const uint32_t *q_offsets,
                                    const uint32_t *q_term_ids, const float *q_weights,
                                    const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                                    const slg_sort_spec *sort_or_null, const slg_bool_spec *bool_or_null,
                                    const slg_phrase_spec *phrases, uint32_t k, int strategy);
int slg_search_batch_phrase(slg_index *index, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                            const float *q_weights, const slg_score_plans *plans_or_null,
                            const int32_t *q_filter_or_null, const slg_sort_spec *sort_or_null,
                            const slg_bool_spec *bool_or_null, const slg_phrase_spec *phrases, uint32_t k,
                            int strategy, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                            uint32_t *out_count, slg_stats *stats_or_null, uint64_t *out_matched_or_null);

/* ---------------------------------------------------------------------------------------------------------
 * function_score at the root of the score tree, with the batch's scored query as its inner query: boost by a
 * column (field_value_factor), by closeness to an origin (decay), by a constant under a filter (weight), and
 * min_score.  The reference visits every accepted doc, computes the node's score from the doc's base score
 * and fast-field values, drops the doc when that gives None and ranks by the computed score
 * (evaluate_compiled_score, api/reader.rs:491-548 and :3166-3187; query/score_functions.rs).  Every candidate
 * passes matches_subquery, because the inner query is the scored one.
 *
 * FUNCTIONS.  Query q has functions q_fn_offsets[q] .. q_fn_offsets[q + 1] - 1 (at most SLG_MAX_FSCORE_FUNCS),
 * evaluated in that order.  Each gives the doc a VALUE (f32) or none.  f_filter is a filter id of
 * slg_index_add_filter* or -1: a function whose filter rejects the doc gives none.
 *   SLG_FSCORE_WEIGHT               the value is f_weight.
 *   SLG_FSCORE_FIELD_VALUE_FACTOR   raw = the FIRST value of the doc in column f_field, or f_missing when the doc
 *                                   has none; scaled = raw * (double)f_weight (the factor); non-finite: no value;
 *                                   m = modifier(scaled); non-finite: no value; the value is (float)m.  Modifiers:
 *                                   NONE x; LOG x <= 0 ? 0 : ln x; LOG1P x <= -1 ? 0 : ln(1 + x) (log1p);
 *                                   LOG2P x <= -1 ? 0 : log2(x + 1); SQRT x < 0 ? 0 : sqrt x;
 *                                   RECIPROCAL x == 0 ? 0 : 1 / x.
 *   SLG_FSCORE_DECAY                a doc without a value in f_field: no value.  distance = |v - f_origin| -
 *                                   f_offset, norm = max(distance, 0) / f_scale; EXP pow(f_decay, norm), GAUSS
 *                                   pow(f_decay, norm * norm), LINEAR max((1 - norm) * (1 - f_decay) + f_decay, 0);
 *                                   non-finite: no value; the value is (float) of it.
 * All of this is f64 arithmetic, operation by operation (no contraction).  Columns are the numeric columns of
 * slg_index_add_agg_field_f64 / _i64 (an i64 value counts `as f64`); a function_score batch only reads them.
 *
 * COMBINE, in f32, operation by operation.  fs = the present values folded left to right by q_score_mode: SUM,
 * MULTIPLY, MAX, MIN (fmaxf / fminf: a NaN operand loses, as Rust's f32::max / min), AVG (the sum divided by the
 * number of present values).  base = the doc's first-pass score; eff = base, but 1.0 when |base| <= FLT_EPSILON
 * and a value is present.  combined = eff when no value is present, else by q_boost_mode: MULTIPLY eff * fs,
 * SUM eff + fs, REPLACE fs, MAX fmaxf(eff, fs), MIN fminf(eff, fs).  Then, in this order: with
 * SLG_FSCORE_HAS_MAX_BOOST combined = fminf(combined, q_max_boost); with SLG_FSCORE_HAS_MIN_SCORE the doc is
 * DROPPED when combined < q_min_score; combined *= q_boost.  A query without functions still applies the three.
 * A dropped doc is not ranked and not counted: slg_stats.scored_docs = the count of the same batch without the
 * spec minus the dropped docs (the bool batch's rule), and a sorted batch's matched counts see survivors only.
 * A query with no function, neither flag and q_boost == 1 is untouched, bit for bit; such queries mix with
 * others in a batch.  (A NaN score has the sign the device's arithmetic gives it.)
 *
 * slg_batch_prepare_fscore is slg_batch_prepare_plans (sort NULL: rows in order of the new score) or
 * slg_batch_prepare_sorted (a field sort; `_score` parts read the new score) plus the spec.  The batch is planned
 * as a sorted batch is — every doc of the scored lists is a candidate with its exact score, no threshold seed,
 * no MaxScore, whatever k is — and slg_batch_run enqueues ONE kernel between the scoring kernel and the select
 * that rewrites every candidate's score and drops those below min_score.  A batch in which no query has work
 * launches nothing.  The kernel has two instantiations, chosen per batch: a lean one for batches whose
 * functions need no ln / log1p / log2 / pow (weight, NONE / SQRT / RECIPROCAL, LINEAR), and a full one;
 * slg_batch_fscore_info tells which (0: nothing is launched, 1 lean, 2 full) and how many queries have work.
 * run / fetch / device_results / sync / set_stream as for any batch; slg_batch_matched_counts for the sorted
 * form.  Columns and filters are those of the index state the batch was prepared on.  slg_search_batch_fscore
 * is the one-call form; stats may be NULL; out_matched may be NULL and must be NULL without a sort spec.
 *
 * Errors, the spec's own before an index state is looked at.  SLG_ERR_INVALID: a NULL spec or array, offsets
 * that decrease, an unknown kind, mode, modifier or decay function, a non-finite weight or factor, a non-finite
 * scale or scale <= 0, f_decay outside (0, 1]; then against the state: an unknown field or filter id, a keyword
 * column, a field without a column for a segment.  SLG_ERR_UNSUPPORTED (CPU scorer): more than
 * SLG_MAX_FSCORE_FUNCS functions in a query, a column that holds a non-finite value (the rule of aggregations).
 * slg_batch_run_sharded* and slg_batch_fetch_sharded refuse a function_score batch with SLG_ERR_UNSUPPORTED.
 * Built beside it: script_score at the root, and the two nodes nested one inside the other
 * (slg_batch_prepare_script, below).  Not built (CPU scorer): function_score below the root or over any other
 * inner query (rank_feature and constant_score at the root are scan batches, below), deeper nesting,
 * (explain is built: slg_batch_explain, at the end of this header), function filters other than registered
 * filter ids, and specs on hybrid, rescore, sharded and coalesced batches
 * (behind bool, phrase or tree clauses, with a cursor, aggregations or collapse:
 * slg_batch_prepare_request, "compound requests" below).
 * --------------------------------------------------------------------------------------------------------- */
#define SLG_MAX_FSCORE_FUNCS 8u /* functions of one query */
enum { SLG_FSCORE_WEIGHT = 0, SLG_FSCORE_FIELD_VALUE_FACTOR = 1, SLG_FSCORE_DECAY = 2 };
enum { SLG_FSCORE_MOD_NONE = 0, SLG_FSCORE_MOD_LOG = 1, SLG_FSCORE_MOD_LOG1P = 2, SLG_FSCORE_MOD_LOG2P = 3,
       SLG_FSCORE_MOD_SQRT = 4, SLG_FSCORE_MOD_RECIPROCAL = 5 };
enum { SLG_FSCORE_DECAY_EXP = 0, SLG_FSCORE_DECAY_GAUSS = 1, SLG_FSCORE_DECAY_LINEAR = 2 };
enum { SLG_FSCORE_MODE_SUM = 0, SLG_FSCORE_MODE_MULTIPLY = 1, SLG_FSCORE_MODE_MAX = 2, SLG_FSCORE_MODE_MIN = 3,
       SLG_FSCORE_MODE_AVG = 4 };
enum { SLG_FSCORE_BOOST_MULTIPLY = 0, SLG_FSCORE_BOOST_SUM = 1, SLG_FSCORE_BOOST_REPLACE = 2,
       SLG_FSCORE_BOOST_MAX = 3, SLG_FSCORE_BOOST_MIN = 4 };
#define SLG_FSCORE_HAS_MAX_BOOST 1u
#define SLG_FSCORE_HAS_MIN_SCORE 2u
typedef struct slg_fscore_spec {
  const uint32_t *q_fn_offsets; /* [nq + 1] into the f_ arrays */
  const int32_t *q_score_mode;  /* [nq] SLG_FSCORE_MODE_* */
  const int32_t *q_boost_mode;  /* [nq] SLG_FSCORE_BOOST_* */
  const uint32_t *q_flags;      /* [nq] SLG_FSCORE_HAS_* */
  const float *q_max_boost;     /* [nq] read with SLG_FSCORE_HAS_MAX_BOOST */
  const float *q_min_score;     /* [nq] read with SLG_FSCORE_HAS_MIN_SCORE */
  const float *q_boost;         /* [nq] */
  const int32_t *f_kind;        /* [n_functions] SLG_FSCORE_WEIGHT / _FIELD_VALUE_FACTOR / _DECAY */
  const int32_t *f_field;       /* [n_functions] agg field id (numeric); not read for a weight */
  const int32_t *f_filter;      /* [n_functions] filter id or -1 */
  const float *f_weight;        /* [n_functions] the weight, or field_value_factor's factor */
  const int32_t *f_modifier;    /* [n_functions] SLG_FSCORE_MOD_* (field_value_factor) */
  const int32_t *f_decay_fn;    /* [n_functions] SLG_FSCORE_DECAY_* (decay) */
  const double *f_missing;      /* [n_functions] field_value_factor: the value of a doc without one */
  const double *f_origin;       /* [n_functions] decay */
  const double *f_scale;        /* [n_functions] decay: finite, > 0 */
  const double *f_offset;       /* [n_functions] decay */
  const double *f_decay;        /* [n_functions] decay: in (0, 1] */
} slg_fscore_spec;
slg_batch *slg_batch_prepare_fscore(slg_index *index, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                                    const float *q_weights, const slg_score_plans *plans_or_null,
                                    const int32_t *q_filter_or_null, const slg_sort_spec *sort_or_null,
                                    const slg_fscore_spec *spec, uint32_t k, int strategy);
int slg_batch_fscore_info(const slg_batch *batch, uint32_t *out_variant, uint32_t *out_queries_with_work);
int slg_search_batch_fscore(slg_index *index, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                            const float *q_weights, const slg_score_plans *plans_or_null,
                            const int32_t *q_filter_or_null, const slg_sort_spec *sort_or_null,
                            const slg_fscore_spec *spec, uint32_t k, int strategy, uint32_t *out_doc, uint32_t *out_seg,
                            float *out_score, uint32_t *out_count, slg_stats *stats_or_null,
                            uint64_t *out_matched_or_null);

/* ---------------------------------------------------------------------------------------------------------
 * script_score at the root of the score tree, with the batch's scored query as its inner query: an arithmetic
 * script over the doc's base score, constants and numeric fast fields (query/script.rs; the node:
 * evaluate_compiled_score, api/reader.rs:577-612; planner.rs:776-791 builds matcher and scorer from the inner
 * node, so every candidate passes matches_subquery).  Optionally chained with a function_score stage: the two
 * nodes nested one inside the other.
 *
 * PROGRAM.  Query q has instructions p_offsets[q] .. p_offsets[q + 1] - 1 (at most SLG_MAX_SCRIPT_INSTRS): the
 * script in reverse Polish order, as CompiledScript holds it, evaluated in f64 on a stack (script.rs:69-146), one
 * correctly rounded operation at a time.
 *   SLG_SCRIPT_PUSH_CONST  push consts[i_arg] (number literals and params: both are constants here)
 *   SLG_SCRIPT_PUSH_FIELD  push the doc's FIRST value of agg column i_arg (slg_index_add_agg_field_f64 / _i64, an
 *                          i64 value `as f64`), or 0.0 when the doc has none (script.rs:80-87)
 *   SLG_SCRIPT_PUSH_SCORE  push the doc's base score `as f64`
 *   SLG_SCRIPT_ADD / _SUB / _MUL   pop b, pop a, push a op b; a non-finite result: NONE
 *   SLG_SCRIPT_DIV         pop b, pop a; b == 0.0 (also -0.0): NONE, before dividing; push a / b; non-finite: NONE
 *   SLG_SCRIPT_NEG         pop a, push -a
 * AFTER THE PROGRAM.  v = (float)top, non-finite: NONE (reader.rs:596); score = v * q_boost in f32, non-finite:
 * NONE (:599-602).  NONE DROPS the doc: it is not ranked and not counted — slg_stats.scored_docs and a sorted
 * batch's matched counts follow the rule of function_score's min_score drops.  A query with no instruction is
 * untouched, bit for bit (its q_boost is checked, not applied); such queries mix with scripted ones in a batch.
 *
 * BOOSTS.  The reference hands a node's incoming boost B on to its inner node and gives the node itself
 * B * node_boost (planner.rs:783-790; function_score the same, :746-755).  The ABI takes FINAL values per stage: the
 * caller folds B into q_weights as for any query, passes q_boost = B * node_boost of the script_score node here and
 * q_boost = B * node_boost of the function_score node in its spec.
 *
 * slg_batch_prepare_script is slg_batch_prepare_fscore with the script spec: planned as a sorted batch is (every doc
 * of the scored lists is a candidate with its exact score), in score order or under a sort spec whose `_score` parts
 * read the new score.  fscore NULL: the script stage alone (`order` must still be one of the two values).  With an
 * fscore spec the batch has two stages, enqueued behind the scoring kernel and in front of the select in this order:
 *   SLG_SCRIPT_OUTER  function_score first, the script reads its score and the docs it dropped stay dropped:
 *                     script_score{query: function_score{query: Q}}
 *   SLG_SCRIPT_INNER  the script first, function_score reads its score: function_score{query: script_score{query: Q}}
 * (evaluate_compiled_score evaluates a node's `base` with `?`: an inner None drops the doc, else the outer node
 * reads the inner score.)  A stage in which no query has work launches nothing.  slg_batch_script_info: the
 * queries with a program and the deepest stack of the batch's programs (0 without work).  slg_batch_fscore_info
 * answers for the fscore stage when there is one.  slg_search_batch_script is the one-call form; stats may be NULL;
 * out_matched may be NULL and must be NULL without a sort spec.
 *
 * Errors, the spec's own before an index state is looked at.  SLG_ERR_INVALID: a NULL spec or array, offsets that
 * decrease, an unknown op, a const index >= n_consts, a non-finite q_boost, an unknown order;
 * then against the state: an unknown field id, a keyword column, a field without a column for a segment.
 * SLG_ERR_UNSUPPORTED (CPU scorer), behind every invalid argument: a program of more than SLG_MAX_SCRIPT_INSTRS
 * instructions, a stack deeper than SLG_MAX_SCRIPT_DEPTH, more than SLG_MAX_SCRIPT_FIELDS distinct fields in a
 * query, a non-finite constant (the reference compiles a 310-digit literal to inf and returns None for every doc),
 * an ill-formed program — a stack underflow or a final depth other than 1, which the reference accepts and answers
 * with no hit (e.g. "1 2") — and a column that holds a non-finite value (the rule of aggregations).
 * slg_batch_run_sharded* and slg_batch_fetch_sharded refuse a script batch with SLG_ERR_UNSUPPORTED.
 * Not built (CPU scorer): script_score below the root or over any other inner query, more than the two stages,
 * and specs on hybrid, rescore, sharded and coalesced batches (explain is built: slg_batch_explain, at the end of
 * this header; rank_feature and constant_score at the root are
 * scan batches, below; behind bool, phrase or tree clauses, with a cursor, aggregations or collapse:
 * slg_batch_prepare_request, "compound requests" below).
 * --------------------------------------------------------------------------------------------------------- */
#define SLG_MAX_SCRIPT_INSTRS 64u /* instructions of one query */
#define SLG_MAX_SCRIPT_DEPTH 8u   /* stack slots */
#define SLG_MAX_SCRIPT_FIELDS 8u  /* distinct fields of one query */
enum { SLG_SCRIPT_PUSH_CONST = 0, SLG_SCRIPT_PUSH_FIELD = 1, SLG_SCRIPT_PUSH_SCORE = 2, SLG_SCRIPT_ADD = 3,
       SLG_SCRIPT_SUB = 4, SLG_SCRIPT_MUL = 5, SLG_SCRIPT_DIV = 6, SLG_SCRIPT_NEG = 7 };
enum { SLG_SCRIPT_OUTER = 0, SLG_SCRIPT_INNER = 1 };
typedef struct slg_script_spec {
  const uint32_t *p_offsets; /* [nq + 1] into the i_ arrays */
  const int32_t *i_op;       /* [n_instructions] SLG_SCRIPT_* */
  const int32_t *i_arg;      /* [n_instructions] PUSH_FIELD: agg field id (numeric); PUSH_CONST: index into consts */
  const double *consts;      /* [n_consts] */
  uint32_t n_consts;
  const float *q_boost;      /* [nq] */
} slg_script_spec;
slg_batch *slg_batch_prepare_script(slg_index *index, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                                    const float *q_weights, const slg_score_plans *plans_or_null,
                                    const int32_t *q_filter_or_null, const slg_sort_spec *sort_or_null,
                                    const slg_script_spec *script, const slg_fscore_spec *fscore_or_null, int order,
                                    uint32_t k, int strategy);
int slg_batch_script_info(const slg_batch *batch, uint32_t *out_queries_with_work, uint32_t *out_max_depth);
int slg_search_batch_script(slg_index *index, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                            const float *q_weights, const slg_score_plans *plans_or_null,
                            const int32_t *q_filter_or_null, const slg_sort_spec *sort_or_null,
                            const slg_script_spec *script, const slg_fscore_spec *fscore_or_null, int order, uint32_t k,
                            int strategy, uint32_t *out_doc, uint32_t *out_seg, float *out_score, uint32_t *out_count,
                            slg_stats *stats_or_null, uint64_t *out_matched_or_null);

/* ---------------------------------------------------------------------------------------------------------
 * Scan batches: match_all, constant_score and rank_feature at the root — requests WITHOUT a scored term.  They
 * bring no posting list, so their candidates come from a scan over every doc of every segment, the reference's
 * scan_segment (api/reader.rs:3131-3236).  Every stage behind the candidates is the one every batch kind runs.
 *
 * MATCH.  A doc matches when it is not deleted, the node's own filter (q_filter of the spec: constant_score.filter,
 * a filter id of slg_index_add_filter* or -1) passes and the batch's root filter (q_filter of the call) passes;
 * docs 0 .. n_docs - 1 of every segment are looked at (:3154-3164).
 * SCORE.
 *   SLG_SCAN_MATCH_ALL     1.0 (:428, :3151).
 *   SLG_SCAN_CONSTANT      q_score: boost * node_boost, multiplied by the caller (:484-490); finite.
 *   SLG_SCAN_RANK_FEATURE  raw = the FIRST value of the doc in column q_field `as f64`, or (double)q_missing when
 *                          the doc has none (:176-181); m = modifier(raw): NONE raw; LOG raw <= 0 ? 0 : ln raw;
 *                          LOG1P raw <= -1 ? 0 : ln(1 + raw) (ln_1p); SQRT raw < 0 ? 0 : sqrt raw; RECIPROCAL
 *                          raw == 0 ? 0 : 1 / raw (:183-215); a non-finite m DROPS the doc; s = (float)m * q_boost
 *                          in f32; a non-finite s DROPS the doc (:549-576).  f64 arithmetic, operation by operation.
 * A dropped doc is neither ranked, counted nor aggregated (the `continue` at :3176-3179 comes before the counter
 * and the collector).
 * ORDER.  Rows as in every batch: in score order (score desc by total_cmp, segment asc, doc asc); under a sort
 * spec the SortKey order of slg_batch_prepare_sorted.  slg_batch_matched_counts gives total_matches for EVERY scan
 * batch — score-ordered ones and k == 0 included; slg_stats.scored_docs and candidates_examined are the same
 * number (postings_advanced is 0).
 * ONE KNOWN DEVIATION.  Under a sort spec without a `_score` part the reference still reports the computed score
 * of a CONSTANT or RANK_FEATURE hit; the sorted select writes 0.0 there, as for every sorted batch, and a scan batch
 * returns 0.0.  (MATCH_ALL is 0.0 there in the reference too, :3151.)
 *
 * slg_batch_prepare_scan: sort_or_null and aggs_or_null mean what they mean in slg_batch_prepare_aggs (all seven
 * aggregation kinds); k == 0 is legal, k <= SLG_MAX_K.  slg_batch_run enqueues scan_kernel — no partition kernel
 * and no scoring kernel — then the select of the batch's order and, with a spec, the aggregation kernels; a batch
 * with k == 0 and no aggregation launches the scan alone.  The kernel has two instantiations, chosen per batch: a
 * lean one (MATCH_ALL, CONSTANT, the modifiers NONE / SQRT / RECIPROCAL) and a full one with the f64 ln / log1p;
 * slg_batch_scan_info tells which (0: the batch has no slice, 1 lean, 2 full), the batch's slices and the docs per
 * slice the planner cuts at.  run / fetch / device_results / matched_counts / agg_layout / fetch_aggs /
 * fetch_agg_values / set_stream / sync as for any batch.  slg_search_batch_scan is the one-call form with the
 * outputs of slg_search_batch_agg_values; the aggregation outputs may be NULL without a spec, out_matched may be
 * NULL.
 * MEMORY.  A query whose kind is MATCH_ALL or CONSTANT, in a batch without sort spec and without aggregations, keeps
 * min(slice docs, k) candidates per slice (all its scores are equal: a doc of the top k is among the first k
 * passing docs of its slice) and counts the rest.  Every other query keeps 8 bytes per doc of every segment; a
 * batch too large for the device fails with SLG_ERR_OOM as any candidates-mode batch does.
 *
 * Errors, all on the host before any device work.  SLG_ERR_INVALID: a NULL spec or array, an unknown kind or
 * modifier, a non-finite q_score (CONSTANT), q_missing or q_boost (RANK_FEATURE), an unknown or incomplete filter
 * id, an unknown field id, a keyword column, a field without a column for every segment, an invalid sort spec or
 * aggregation spec.  SLG_ERR_UNSUPPORTED: a column recorded as holding a non-finite value (the rule of
 * aggregations), k > SLG_MAX_K; slg_batch_run_sharded* and slg_batch_fetch_sharded refuse a scan batch.
 * Not built (CPU path): scan batches with cursor, collapse, rescore, hybrid, function_score or script_score over
 * them, scan requests in the coalescer, and scan queries mixed with scored queries in one batch.
 * --------------------------------------------------------------------------------------------------------- */
enum { SLG_SCAN_MATCH_ALL = 0, SLG_SCAN_CONSTANT = 1, SLG_SCAN_RANK_FEATURE = 2 };
enum { SLG_SCAN_MOD_NONE = 0, SLG_SCAN_MOD_LOG = 1, SLG_SCAN_MOD_LOG1P = 2, SLG_SCAN_MOD_SQRT = 3,
       SLG_SCAN_MOD_RECIPROCAL = 4 };
typedef struct slg_scan_spec {
  const int32_t *q_kind;     /* [nq] SLG_SCAN_* */
  const int32_t *q_filter;   /* [nq] the node's own filter id, or -1 */
  const float *q_score;      /* [nq] CONSTANT: boost * node_boost */
  const int32_t *q_field;    /* [nq] RANK_FEATURE: agg field id (numeric) */
  const int32_t *q_modifier; /* [nq] RANK_FEATURE: SLG_SCAN_MOD_* */
  const float *q_missing;    /* [nq] RANK_FEATURE */
  const float *q_boost;      /* [nq] RANK_FEATURE */
} slg_scan_spec;
slg_batch *slg_batch_prepare_scan(slg_index *index, uint32_t nq, const slg_scan_spec *spec,
                                  const int32_t *q_filter_or_null, const slg_sort_spec *sort_or_null,
                                  const slg_agg_spec *aggs_or_null, uint32_t k);
int slg_batch_scan_info(const slg_batch *batch, uint32_t *out_variant, uint32_t *out_slices, uint32_t *out_slice_docs);
int slg_search_batch_scan(slg_index *index, uint32_t nq, const slg_scan_spec *spec, const int32_t *q_filter_or_null,
                          const slg_sort_spec *sort_or_null, const slg_agg_spec *aggs_or_null, uint32_t k,
                          uint32_t *out_doc, uint32_t *out_seg, float *out_score, uint32_t *out_count,
                          uint64_t *out_matched_or_null, uint64_t *counts, slg_agg_stats *stats, uint64_t *values);

/* ---- field collapsing (SearchRequest::collapse, api/reader.rs:2826-2835, 3499-3595) --------------------
 * The reference collapses the top_k = candidate_size + 1 hits it already holds, in their SortKey order
 * (collapse_hits): a hit without a value of the collapse field is dropped (it is in no group and nobody's
 * inner hit), a hit with more than one value fails the request, every other hit joins the group of its value;
 * groups are ordered by first appearance, a group's first hit is its representative and the rest are its
 * members; total_groups counts the groups over those hits, the caller truncates the representatives to
 * `limit` and takes next_cursor from the limit-th.  With inner_hits the members (never the representative)
 * are put in the inner sort's order when that differs from the request's — a full SortKey, so ties after all
 * parts go to segment asc, doc asc — then the first `from` are dropped and at most `size` kept.
 *
 * A collapse batch is slg_batch_prepare_plans (sort_or_null == NULL and q_cursor_or_null == NULL),
 * slg_batch_prepare_sorted (a sort) or slg_batch_prepare_after (a cursor) with one collapse spec for the
 * whole batch; its rows (slg_batch_fetch, slg_batch_device_results) are bit-identical to the same batch
 * without the spec.  One more kernel behind the batch's last one collapses each query's rows on the device
 * into side arrays that slg_batch_fetch_collapse copies out; running the batch again computes them again.
 * The group keys are the global ordinals of a keyword column (slg_index_add_agg_field_ord).
 *
 * Per query q with n = out_count[q] rows: total_groups[q] = groups over the n rows; n_groups[q] =
 * min(total_groups[q], group_limit); for g < n_groups[q] (arrays [nq x group_limit]): group_row = the
 * representative's index among the query's rows, group_doc / group_seg / group_score = that row, group_ord =
 * its ordinal, group_size = rows of the group, the representative included, inner_count = kept members =
 * min(inner_size, max(0, group_size - 1 - inner_from)); inner_row / inner_doc / inner_seg / inner_score
 * ([nq x group_limit x inner_size]) = the kept members in inner order, inner_row indexing the query's rows.
 * status[q] = 1 if one of the n rows has more than one value in the column (the caller fails that request,
 * as the reference does), else 0.  Everything past a count is zero; for a query with status 1 every other
 * output is zero.  Every output pointer may be NULL.
 *
 * inner_sort: NULL = the batch's own order (members stay in row order); else up to SLG_MAX_SORT_PARTS parts
 * as in slg_sort_spec (n_parts == 0 = `_score` desc, what the reference resolves an empty inner sort to,
 * query/sort.rs:159-167).  A `_score` part reads the row's score: 0.0 in a field sort without a `_score`
 * part (ScoreMode::MatchOnly, api/reader.rs:2936-2940).
 *
 * Checked before any device work.  SLG_ERR_INVALID: collapse NULL; group_limit == 0 or > k; an inner sort
 * part with an unknown order or a negative field other than SLG_SORT_SCORE; against the index: an unknown
 * field id, a numeric agg field, a field without a column for every segment, an unknown inner sort field.
 * SLG_ERR_UNSUPPORTED (CPU path): k > SLG_MAX_COLLAPSE_ROWS; inner_size > 0 and inner_from + inner_size >
 * SLG_MAX_INNER_HITS; more than SLG_MAX_SORT_PARTS inner parts.  slg_batch_fetch_collapse on another kind
 * of batch or before the batch has run: SLG_ERR_INVALID.  NOT BUILT: collapse together with
 * rescore, hybrid or vector-only batches (behind clause and score stages and beside aggregations:
 * slg_batch_prepare_request, "compound requests" below), in the coalescer or sharded
 * (slg_batch_run_sharded* and slg_batch_fetch_sharded refuse a collapse batch: SLG_ERR_UNSUPPORTED);
 * k > SLG_MAX_COLLAPSE_ROWS; inner_hits beyond SLG_MAX_INNER_HITS (an unlimited inner size included). */
#define SLG_MAX_COLLAPSE_ROWS 4096u /* k of a collapse batch: the rows of a query are collapsed in LDS */
#define SLG_MAX_INNER_HITS 64u      /* inner_from + inner_size: one member per lane of a wave */
typedef struct slg_collapse_spec {
  int32_t field;        /* id of a KEYWORD column (slg_index_add_agg_field_ord): global ordinals = group keys */
  uint32_t group_limit; /* groups reported per query (the request's limit), 1 .. k */
  uint32_t inner_from;
  uint32_t inner_size;  /* 0 = no inner hits */
  const slg_sort_spec *inner_sort; /* NULL: the batch's own order */
} slg_collapse_spec;
slg_batch *slg_batch_prepare_collapse(slg_index *index, uint32_t nq, const uint32_t *q_offsets,
                                      const uint32_t *q_term_ids, const float *q_weights,
                                      const slg_score_plans *plans_or_null, const int32_t *q_filter_or_null,
                                      const slg_sort_spec *sort_or_null, const slg_sort_cursor *q_cursor_or_null,
                                      const slg_collapse_spec *collapse, uint32_t k, int strategy);
/* The collapse arrays of the batch's last run; waits for the batch. */
int slg_batch_fetch_collapse(slg_batch *batch, uint32_t *n_groups, uint32_t *total_groups, uint32_t *status,
                             uint32_t *group_row, uint32_t *group_ord, uint32_t *group_size, uint32_t *group_doc,
                             uint32_t *group_seg, float *group_score, uint32_t *inner_count, uint32_t *inner_row,
                             uint32_t *inner_doc, uint32_t *inner_seg, float *inner_score);
/* One-call form with host arrays: the rows as slg_batch_fetch, then the arrays of slg_batch_fetch_collapse. */
int slg_search_batch_collapse(slg_index *index, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                              const float *q_weights, const slg_score_plans *plans_or_null,
                              const int32_t *q_filter_or_null, const slg_sort_spec *sort_or_null,
                              const slg_sort_cursor *q_cursor_or_null, const slg_collapse_spec *collapse, uint32_t k,
                              int strategy, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                              uint32_t *out_count, uint32_t *n_groups, uint32_t *total_groups, uint32_t *status,
                              uint32_t *group_row, uint32_t *group_ord, uint32_t *group_size, uint32_t *group_doc,
                              uint32_t *group_seg, float *group_score, uint32_t *inner_count, uint32_t *inner_row,
                              uint32_t *inner_doc, uint32_t *inner_seg, float *inner_score);

/* ---- compound requests: several batch kinds in one batch ------------------------------------------------
 * A SearchRequest is rarely one feature: a filtered bool query with facets, a function_score around a bool,
 * a bool under a sort with search_after, collapse over a phrase query.  slg_batch_prepare_request takes the
 * query arrays of slg_batch_prepare_plans and one nullable pointer per kind; a kind is asked for when its
 * pointer is non-NULL (script_order is read only with script_spec).  Every slg_batch_prepare_<kind> is this
 * call with that kind's pointers set: a request that asks for one kind gives that kind's batch, byte for byte.
 * The batch is an ordinary slg_batch: slg_batch_run / _fetch / _matched_counts / _cursor_seen, and the fetches
 * of every kind it was asked for (slg_batch_fetch_aggs, _agg_values, _top_hits, _composite with
 * slg_batch_set_composite_after, _term_buckets, _rescore, _collapse, slg_batch_highlight).  There is no
 * one-call form.
 *
 * ORDER OF THE STAGES (one run; each stage is the kernel of its kind, unchanged).  Per candidate the reference
 * runs score_adjust (which may drop the doc), then accept (tombstones, matcher, root filter, cursor, matched
 * count), then collector.collect (query/wand.rs:506-517; the collectors are fed from accept's survivors,
 * api/reader.rs:3020-3028).  The device runs: scoring; the clause stage (drops the candidates the matcher
 * rejects); the score stage (function_score / script_score, in script_order: rewrites every surviving
 * candidate's score, drops those below min_score or without a script value); the select in score order or
 * under the sort, with the cursor; the collectors over the surviving candidates; rescore or collapse over the
 * rows.  The matcher never reads a score and the score stage never reads the matcher, so clause-then-score
 * keeps exactly the docs score_adjust-then-matcher keeps.
 *
 * THE MATCHED SET of a compound batch is the docs that pass tombstones, q_filter, the clause stage and the
 * score stage's min_score.  slg_batch_matched_counts, the aggregation tables, top_hits, composite,
 * term buckets and collapse's total_groups (over the rows) see exactly that set; top_hits and a `_score` sort
 * part see the rewritten score; the rows equal those of the same request without collectors / collapse, bit
 * for bit.  slg_stats.scored_docs is the plain batch's count minus the clause stage's rejects minus the score
 * stage's drops (each stage takes its own off the same counter, over the candidates the stage before left).
 *
 * LEGAL COMBINATIONS.
 *   clause stage   at most one of bool_spec, phrase_spec (with its optional bool_spec: the term groups of a
 *                  phrase batch, as slg_batch_prepare_phrase) and bool_tree_spec
 *   score stage    fscore_spec, script_spec, or both in script_order; alone or behind a clause stage
 *                  (function_score{query: bool{..}} / script_score{query: bool{..}} at the root)
 *   order          score order or sort, q_cursor on either; behind any clause and / or score stage
 *   collectors     aggs, alone or with ONE of top_hits / composite / term_buckets (each of the three also
 *                  without aggs), behind any clause and / or score stage, in score order or under a sort
 *   collapse       k <= SLG_MAX_COLLAPSE_ROWS, SLG_MAX_INNER_HITS inner hits; behind any clause and / or score
 *                  stage, beside collectors, and with a cursor when there are no collectors
 *   rescore        score order, no cursor; alone or behind a clause stage
 * REFUSED, SLG_ERR_UNSUPPORTED (CPU path), the message naming the pair, before the index is looked at and after
 * every kind's own argument checks (an invalid argument is reported before an unsupported combination):
 *   bool_tree_spec with bool_spec or phrase_spec (two clause kinds);
 *   two of top_hits / composite / term_buckets;
 *   q_cursor with aggs, top_hits, composite or term_buckets: the reference collects only the docs behind the
 *     cursor (accept returns false before collector.collect) and the collectors' walks do not test the cursor;
 *   rescore with sort, q_cursor, fscore_spec, script_spec, aggs, top_hits, composite, term_buckets or collapse.
 * Hybrid, vector-only and scan batches are not requests of this form: they keep their own entry points
 * (slg_batch_prepare_hybrid, slg_vector_search_batch*, slg_batch_prepare_scan) and the struct cannot ask for
 * them.  The coalescer takes plain requests only, and slg_batch_run_sharded* / slg_batch_fetch_sharded refuse
 * a compound batch by the first of its kinds they do not run (SLG_ERR_UNSUPPORTED).
 *
 * SLG_ERR_INVALID: req NULL; struct_size other than sizeof(slg_request) (the struct may grow: always set it
 * from sizeof); reserved other than 0; index NULL; and whatever each kind's own prepare call reports for its spec, with the same
 * message.  Each kind's limits (SLG_MAX_*) hold as in its own section. */
typedef struct slg_request {
  uint32_t struct_size; /* = sizeof(slg_request) */
  uint32_t nq;
  const uint32_t *q_offsets;  /* the query arrays of slg_batch_prepare_plans */
  const uint32_t *q_term_ids;
  const float *q_weights;
  const slg_score_plans *plans; /* NULL: every query is a flat sum */
  const int32_t *q_filter;      /* NULL: no query is filtered */
  uint32_t k;
  int32_t strategy;
  const slg_sort_spec *sort;                /* NULL: score order */
  const slg_sort_cursor *q_cursor;          /* [nq]; NULL: no cursor */
  const slg_bool_spec *bool_spec;           /* clause stage: bool (with phrase_spec: its term groups) */
  const slg_phrase_spec *phrase_spec;       /* clause stage: phrase */
  const slg_bool_tree_spec *bool_tree_spec; /* clause stage: matcher tree */
  const slg_fscore_spec *fscore_spec;       /* score stage: function_score */
  const slg_script_spec *script_spec;       /* score stage: script_score */
  int32_t script_order;                     /* SLG_SCRIPT_OUTER / _INNER; read only with script_spec */
  uint32_t reserved;                        /* must be 0 */
  const slg_agg_spec *aggs;
  const slg_top_hits_spec *top_hits;
  const slg_composite_spec *composite;
  const slg_term_bucket_spec *term_buckets;
  const slg_rescore_spec *rescore;
  const slg_collapse_spec *collapse;
} slg_request;
slg_batch *slg_batch_prepare_request(slg_index *index, const slg_request *req);

/* ---- term expansion: fuzzy, prefix, wildcard and regex (api/reader.rs:1119-1373, 1394-1465) -----------
 * A request whose terms must be expanded against the term dictionary (SearchRequest.fuzzy, QueryNode::Prefix,
 * QueryNode::Wildcard, QueryNode::Regex) becomes a plain batch once its terms are known: slg_expand_batch returns, per source term,
 * the keys the reference's expansion yields, in its order, as rows of per-segment term ids with their edit
 * distance; the caller weights them (fuzzy: boost * 1 / (distance + 1) in f32, distance_weight, :977-979; prefix,
 * wildcard and regex: boost), folds equal keys of a query by summing (:2971-2983), gives all expansions of a source term
 * that term's plan leaf and prepares an ordinary batch.  Scoring is untouched.
 *
 * DICTIONARIES.  slg_index_set_terms attaches segment seg's dictionary: key_offsets is uint32_t[n_terms + 1] over
 * key_bytes, key i the UTF-8 "field:term" key of term id i of the segment's CSR (n_terms = slg_segment_desc.n_terms).
 * The arrays are borrowed for the call.  The library sorts the keys by bytes (the identity for files written by
 * searchlite, whose dictionary is a BTreeMap, util/fst.rs:25-33), keeps the sorted position -> term id map and a
 * host copy, and stages sorted bytes, offsets, map, a char count per key (u8, saturating) and each key's doc
 * frequency (u32, the length of its posting list as staged; slg_suggest_batch reads it) on the device.  It
 * builds the next index state as slg_index_set_positions does: prepared batches keep theirs;
 * slg_index_update_deleted keeps the dictionaries; a segment added later has none until it is set;
 * slg_index_remove_segment drops its dictionary.  SLG_ERR_INVALID: NULL arrays, seg out of range, decreasing
 * offsets, duplicate keys, a key without ':', invalid UTF-8.
 *
 * REQUESTS.  field and term are UTF-8 with byte lengths (an embedded NUL is a byte like any other: the structs
 * carry lengths, nothing is NUL-terminated); term is already analysed by the caller, as expand_term_groups hands
 * it on (:1020-1099).  Lengths, prefixes and edits are counted in Unicode scalar values, never bytes.  "The
 * range of P" below is terms_with_prefix("field:" + P): the segment's keys that start with it, in byte order; the
 * key "field:" itself is always skipped (:1187, :1257, :1431).
 *
 * FUZZY (:1394-1465).  Key 0 is the exact key "field:term" at distance 0, also when no segment holds it (a row
 * of SLG_NO_TERM).  A term of fewer than min_length chars, max_expansions == 0, or max_edits == 0 (:1140-1143):
 * that is all.  max_edits is clamped to 2.  Then, segment by segment and over the range of the term's first
 * min(prefix_length, chars of the term) chars: skip a candidate equal to the term, one whose char count differs
 * from the term's by more than max_edits, one whose Levenshtein distance (bounded_levenshtein, :981-1018: unit
 * insert / delete / substitute, a transposition is 2) exceeds max_edits, and a key already seen; anything else is
 * a new expansion with its distance.  The cap is GLOBAL: everything stops at max_expansions new keys.
 *
 * PREFIX (:1164-1210) and WILDCARD (:1212-1283).  Every key of the range of the prefix (wildcard: of the
 * pattern's literal prefix, the chars before its first '*' or '?') whose term matches (prefix: always; wildcard:
 * the whole term against the pattern, '*' = any run of chars, '?' = one char, neither matches U+000A because
 * the reference compiles them to the regex '.', every other char is literal) and that no EARLIER segment
 * yielded is an expansion at distance 0.  The cap is PER SEGMENT and counts only such new keys: a key past the cap
 * in segment 0 can still enter through segment 1.  max_expansions == 0: no keys.
 *
 * REGEX (QueryNode::Regex, expand_regex :1322-1373; kind SLG_EXPAND_REGEX = 4; kind 3 is reserved and stays an
 * unknown kind).  term is the pattern, already normalised by the caller as a wildcard pattern is; max_edits,
 * prefix_length and min_length are ignored.  It is expand_wildcard's loop with another predicate and another
 * prefix rule: max_expansions == 0 gives no keys; segments in order; within a segment the range of the pattern's
 * literal prefix in byte order; the key "field:" skipped (:1347); a key passes when ^(?:pattern)$ matches the
 * WHOLE term (util/regex.rs, is_match under the regex crate's defaults: Unicode on, case-sensitive, '.' = any
 * scalar value but U+000A); a key of an earlier segment is skipped (:1354); the cap is PER SEGMENT and counts
 * only new keys (:1344), so R = (seg + 1) * max_expansions as for wildcard.
 *   The literal prefix (regex_literal_prefix, :1285-1320) works on the pattern's TEXT, not on its meaning.
 * Outside an escape: '\' starts an escape (:1310); '^' is dropped while the prefix is still empty (:1311); any of
 * . * + ? ( ) [ ] { } | $ ends the prefix (:1312); any other char is appended (:1313-1316).  After a '\': any of
 * d D w W s S b B p P ends the prefix (:1299-1300); any other char is appended AS ITSELF (:1291-1306), '\\'
 * included, and letters that are escapes in the regex too.  The consequences are the reference's answers and
 * ours: `ab|cd` scans only the range of "ab" and never yields "cd"; `rust?` scans the range of "rust" and never
 * yields "rus"; `ab*` never yields "a"; `\n.*` scans the range of the letter "n" (and so yields nothing).
 *   The pattern is compiled on the host to a minimised byte-level DFA (at most SLG_MAX_REGEX_STATES states with
 * the dead state, at most SLG_MAX_REGEX_TABLE bytes of states x byte classes) that the device walks, a lane per
 * key.  A pattern is never mis-compiled: what is outside the language below is SLG_ERR_UNSUPPORTED (CPU path),
 * whether or not the regex crate would accept it.  An invalid or unsupported pattern is reported whatever
 * max_expansions is (the reference's planner compiles the pattern first, query/planner.rs:599).
 *   Supported: literal chars of any UTF-8 width (']' and '}' alone included); '\' followed by ASCII punctuation
 * other than '<' and '>', as that literal; \n \t \r; '.'; classes [...] and [^...] of single chars and a-z
 * ranges, a leading ']' and a leading or trailing '-' as literals, the same escapes inside, negation over all
 * scalar values, U+000A included; groups ( ), (?: ), (?P<name> ) and (?<name> ) with names of [A-Za-z_][A-Za-z0-9_]*;
 * '|', empty alternatives included; the quantifiers * + ? {n} {n,} {n,m}, each optionally followed by one '?'
 * (lazy: without meaning for a whole-term match); the anchors ^ $ \A \z anywhere in the pattern (a start anchor
 * behind a consumed char, or an end anchor in front of one, matches nothing: `a^b` is empty, `a$|b` is {a, b}).
 *   SLG_ERR_UNSUPPORTED, the message naming the construct and its byte offset: \d \D \w \W \s \S \p \P \b \B
 * (their Unicode tables belong to the regex crate's Unicode version, which cannot be pinned from here); every
 * other alphanumeric escape (\x, \u, octal, ...), '\<', '\>' and '\' before a char that is not ASCII punctuation;
 * any flag group ((?i), (?s), (?x), (?-u), ...) or look-around; a '[' inside a class (nested classes,
 * [:alpha:]); && -- ~~ inside a class; a '-' after a leading ']' in a class; {,m}; a quantifier applied directly
 * to a quantifier (a**, a+*, a{2}{3}, a?+) or to an anchor (^*; a group around the anchor is taken); a repetition count above 1000, groups nested deeper than 32, an
 * automaton of more than 8192 states before minimisation; a minimised DFA above either limit.
 *   SLG_ERR_INVALID (the reference errors too): unbalanced '(' or ')'; an unclosed '['; a reversed range such as
 * [z-a]; a quantifier with nothing to repeat (at the start, after '(' or after '|'); a '{' after an atom that
 * does not complete to {n}, {n,} or {n,m}; {n,m} with n > m; a trailing lone '\'; an empty, unclosed or
 * duplicate group name.
 *
 * OUTPUT.  out_offsets [n_reqs + 1]: request r's keys are rows out_offsets[r] .. out_offsets[r + 1] - 1 of
 * out_term_ids ([rows x n_segs], laid out as q_term_ids: SLG_NO_TERM where the segment lacks the key) and
 * out_distance ([rows] u8).  key_capacity = the rows the two arrays hold.  Size query: out_term_ids and
 * out_distance both NULL fills out_offsets only.  The call is synchronous (as slg_search_batch) and its answer
 * is the same from run to run: the device's rows come from ballots and prefix counts in dictionary order.
 *
 * The device scans (slg_expand.hpp: per request and segment the first R keys of the range that pass the
 * request's predicate, in dictionary order, with their distance); the host runs the reference's sequential loop
 * over those rows (seen set, caps, term-id rows).  R = max_expansions for fuzzy and (seg + 1) * max_expansions
 * for prefix / wildcard / regex is all the reference can consume in a segment.
 *
 * SLG_ERR_INVALID: index, reqs (n_reqs > 0) or out_offsets NULL; a struct_size other than
 * sizeof(slg_expand_req); an unknown kind; field or term NULL with a non-zero length; field or term not valid
 * UTF-8; an invalid regex pattern; a segment without a dictionary; out_term_ids or out_distance NULL but not both;
 * key_capacity too small.
 * SLG_ERR_UNSUPPORTED (CPU path): a term or pattern of more than SLG_MAX_EXPAND_CHARS chars; max_expansions above
 * SLG_MAX_EXPANSIONS; a regex pattern outside the supported language or above the DFA limits (REGEX above).  NOT
 * BUILT: Unicode perl classes, case-insensitive matching and flag groups in a regex (refused, not approximated);
 * unscored (score == false) groups; a query whose folded list
 * exceeds SLG_MAX_QUERY_TERMS (the scoring kernels' cap is untouched); expansion inside sharded or coalesced
 * paths (expand first, then submit the plain query). */
enum { SLG_EXPAND_FUZZY = 0, SLG_EXPAND_PREFIX = 1, SLG_EXPAND_WILDCARD = 2, SLG_EXPAND_REGEX = 4 }; /* 3: reserved */
#define SLG_MAX_EXPAND_CHARS 128u  /* chars of a term or pattern: they sit in LDS beside the scan */
#define SLG_MAX_EXPANSIONS 1024u   /* max_expansions of a request */
#define SLG_MAX_REGEX_STATES 256u  /* states of a pattern's minimised DFA, the dead state included: a transition is a byte */
#define SLG_MAX_REGEX_TABLE 16384u /* states x byte classes: the bytes of its transition table in LDS */
/* the scan's geometry (the boundaries its tests sit on): lanes of a wave = candidate keys looked at together,
 * threads of a workgroup, keys of a range one workgroup scans */
#define SLG_EXPAND_WAVE 64u
#define SLG_EXPAND_WORKGROUP 256u
#define SLG_EXPAND_CHUNK 1024u
typedef struct slg_expand_req {
  uint32_t struct_size;    /* sizeof(slg_expand_req) */
  int32_t kind;            /* SLG_EXPAND_* */
  const char *field;       /* UTF-8, field_len bytes */
  const char *term;        /* UTF-8, term_len bytes: the analysed term, the prefix, the wildcard or regex pattern */
  uint32_t field_len, term_len;
  uint32_t max_expansions;
  uint32_t max_edits, prefix_length, min_length; /* fuzzy only (FuzzyOptions); ignored by the other kinds */
} slg_expand_req;
int slg_index_set_terms(slg_index *index, uint32_t seg, const char *key_bytes, const uint32_t *key_offsets);
int slg_expand_batch(slg_index *index, const slg_expand_req *reqs, uint32_t n_reqs, uint32_t *out_offsets,
                     uint32_t key_capacity, uint32_t *out_term_ids, uint8_t *out_distance);
/* DIAGNOSTIC ONLY, not part of the product path (tools/expand_time.py reads it; a caller has no use for it):
 * where the calling thread's last slg_expand_batch spent its time, in ms, by the host clock: the device scan
 * (uploads, both kernels, the copy back, the wait) and the host merge.  The figures are per thread, not per index:
 * `index` is only checked for NULL.  Either pointer may be NULL. */
int slg_expand_phase_ms(slg_index *index, double *scan_ms, double *merge_ms);

/* ---- completion suggester: prefix and fuzzy, scored by doc frequency (api/reader.rs:1779-1998) ----------
 * SuggestRequest::Completion { field, prefix, size, fuzzy } -> SuggestOption { text, score, doc_freq }: the
 * terms of a field that start with (or lie within a few edits of) what the user has typed, the most frequent
 * first.  slg_suggest_batch answers a batch of independent requests in one call against the dictionaries of
 * slg_index_set_terms, which also stages each key's doc frequency.  Scan AND merge run on the device; the host
 * copies the winners' texts out of its dictionary copy and computes no score, distance or comparison.
 *
 * REQUESTS.  field and term are UTF-8 with byte lengths, as in slg_expand_req.  term is already analysed by the
 * caller (completion_inputs, :1915-1939, always yields exactly one input): for a text field the last token of the
 * analysed prefix, or the raw prefix if there is none; for a keyword field to_ascii_lowercase of the prefix.  It
 * may be empty.  Everything is counted in Unicode scalar values.  size == 0: no options (:1948).
 *
 * DOC FREQUENCY.  df of a key in a segment is the length of its posting list as staged: term_offsets[t + 1] -
 * term_offsets[t] of the slg_segment_desc (PostingsReader::len(), whatever has been deleted since).  So
 * slg_index_update_deleted never changes an answer.
 *
 * PLAIN (has_fuzzy == 0; :1798-1826).  cap = clamp(size * 5, SLG_SUGGEST_MIN_SCAN, SLG_MAX_SUGGEST_CANDIDATES).
 * Segment by segment, over the range of the term in byte order: skip the key "field:" itself; skip a key of df 0
 * without counting it; else options[text].doc_freq += df, options[text].score += (float)df, and the visit counts.
 * The cap is GLOBAL and counts VISITS (the same text in three segments counts three times); everything stops when
 * it is reached.
 *
 * FUZZY (has_fuzzy != 0; FuzzyOptions; :1827-1874).  No options if the term has fewer than min_length chars,
 * max_expansions == 0 or max_edits == 0; max_edits is clamped to 2 first.  cap = max(min(max_expansions,
 * SLG_MAX_SUGGEST_CANDIDATES), size).  Over the range of the term's first min(prefix_length, chars) chars: skip
 * the bare key, a key whose char count differs from the term's by more than max_edits, one whose Levenshtein
 * distance d exceeds max_edits, one of df 0.  A candidate EQUAL to the term passes at distance 0 (unlike
 * slg_expand_batch).  score += (1.0f / (d + 1.0f)) * (float)df: one f32 multiply, then one f32 add, in segment
 * order.  The cap is global and counts visits, as above.
 *
 * RESULT.  Per request the options by score descending, then text ascending in byte order, cut to size;
 * doc_freq is the u64 sum.  Scores, order and doc_freq are the reference's bit for bit, the same from run to run.
 *
 * OUTPUT.  out_offsets [n_reqs + 1]: request r's options are rows out_offsets[r] .. out_offsets[r + 1] - 1 of
 * out_score (f32), out_doc_freq (u64) and out_text_offsets; option i's text is out_text[out_text_offsets[i] ..
 * out_text_offsets[i + 1]): UTF-8 without the "field:" part, not NUL-terminated.  option_capacity = the rows
 * out_score and out_doc_freq hold (out_text_offsets holds option_capacity + 1), text_capacity = the bytes of
 * out_text.  The call is synchronous.
 * SIZE QUERY: out_score, out_doc_freq, out_text_offsets and out_text all NULL.  Then out_offsets must hold
 * n_reqs + 2 entries: [0 .. n_reqs] are filled as above and out_offsets[n_reqs + 1] receives the text bytes the
 * batch needs; the capacities are ignored.  (A caller who knows its longest key can skip it: a request yields at
 * most min(size, SLG_MAX_SUGGEST_CANDIDATES) options.)
 *
 * SLG_ERR_INVALID: index, reqs (n_reqs > 0) or out_offsets NULL; a struct_size other than
 * sizeof(slg_suggest_req); field or term NULL with a non-zero length; field or term not valid UTF-8; a segment
 * without a dictionary; some but not all of the four output arrays NULL; option_capacity or text_capacity too
 * small.  SLG_ERR_UNSUPPORTED (CPU path): a term of more than SLG_MAX_EXPAND_CHARS chars; a fuzzy request whose
 * cap exceeds SLG_MAX_SUGGEST_CANDIDATES, which means size above it (a plain request may have any size: it never
 * yields more than SLG_MAX_SUGGEST_CANDIDATES options).  NOT BUILT: suggest through the coalescer or shard
 * groups; analysis of the prefix. */
#define SLG_MAX_SUGGEST_CANDIDATES 256u /* MAX_SUGGEST_CANDIDATES: the most visits of one request */
#define SLG_SUGGEST_MIN_SCAN 64u        /* DEFAULT_SUGGEST_SCAN: a plain request's smallest cap */
#define SLG_SUGGEST_MERGE_WORKGROUP 256u /* threads of the merge kernel: one per candidate of a request */
typedef struct slg_suggest_req {
  uint32_t struct_size;    /* sizeof(slg_suggest_req) */
  const char *field;       /* UTF-8, field_len bytes */
  const char *term;        /* UTF-8, term_len bytes: the analysed completion input */
  uint32_t field_len, term_len;
  uint32_t size;
  uint32_t has_fuzzy;      /* 0: plain; else the four FuzzyOptions below hold */
  uint32_t max_edits, prefix_length, max_expansions, min_length;
} slg_suggest_req;
int slg_suggest_batch(slg_index *index, const slg_suggest_req *reqs, uint32_t n_reqs, uint32_t *out_offsets,
                      uint32_t option_capacity, float *out_score, uint64_t *out_doc_freq, uint32_t *out_text_offsets,
                      uint32_t text_capacity, char *out_text);
/* DIAGNOSTIC ONLY (tools/suggest_time.py): where the calling thread's last slg_suggest_batch spent its time, in
 * ms, by the host clock: the device part (uploads, the scan's two kernels, the merge kernel, the copy back, the
 * wait) and the host's copy of the texts.  Per thread; `index` is only checked for NULL; either may be NULL. */
int slg_suggest_phase_ms(slg_index *index, double *device_ms, double *copy_ms);

/* ---- highlighting: fragments and tags over registered texts (index/highlight.rs:11-80; api/reader.rs:3400-3497) --
 * materialize_hit reads each hit's stored text and runs highlight_fragments over it: for SearchRequest.highlight
 * per configured field (HighlightOptions: pre_tag, post_tag, fragment_size, number_of_fragments), for
 * highlight_field through make_snippet ("**", "**", 120, 1; the last fragment is the snippet).  Here the texts of
 * a field are registered with the index and one call highlights every (hit, field) of a batch of queries on the
 * device; out_text holds the FINISHED strings, tags inserted.  The host never touches a text.
 *
 * TEXT FIELDS.  slg_index_add_text_field(index, seg_offsets, seg_bytes) -> text field id (>= 0) or a negative
 * error code.  Per segment of the current state u64 offsets[n_docs + 1] and the bytes they index: doc d's text is
 * bytes[offsets[d] .. offsets[d + 1]).  A doc without the field, or with a value that is no string, has an empty
 * text (the reference gives both no entry).  A segment without the field passes NULL offsets.  The call copies
 * bytes[offsets[0] .. offsets[n_docs]) to the device, padded so that a 16-byte load at any doc's last byte stays
 * inside the allocation, and records one bit per doc: "holds a byte >= 0x80".  The texts are part of the immutable
 * index state and follow updates as the other registered columns do: slg_index_update_deleted leaves them alone,
 * slg_index_remove_segment drops the segment's store and the others keep theirs under their new ordinals, a
 * segment added later (slg_index_add_segment) has no text in the field (SLG_HL_NO_TEXT) until the field is
 * registered again over all segments; ids are never handed out again.  slg_index_remove_text_field drops a field
 * (batches prepared before keep it).  SLG_ERR_INVALID: NULL index or seg_offsets, offsets that decrease, NULL bytes
 * under non-empty offsets, an unknown id; SLG_ERR_UNSUPPORTED: a doc of 2^31 bytes or more.
 *
 * WHAT IS COMPUTED (highlight.rs:17-64).  The pattern is `\bw1\W+w2...\b` for each phrase, then `\bterm\b` for
 * each term, joined by `|`, case-insensitive, leftmost-first.  An empty text or no alternative: no fragments.
 * Else offset = 0 and number_of_fragments times: m = the first match in the whole text starting at or after offset
 * (none: stop); start = m.start - min(m.start, fragment_size / 2), end = min(len, start + fragment_size); the
 * fragment text[start .. end) is taken as a string of its own (its edges are text edges) and every non-overlapping
 * match in it, left to right, is wrapped in pre_tag .. post_tag; offset = m.end.  So fragments may overlap and
 * repeat matches, fragment_size 0 yields one empty string per match, and a fragment's edge can cut a word into one
 * that matches another term.  THE DEVICE BUILDS THE WORD-ONLY CASE: ASCII texts, terms and phrase words of one or
 * more bytes of [0-9A-Za-z_].  Then a match is exactly a maximal run of word bytes equal to a term under ASCII case
 * folding, a phrase match as many consecutive runs with anything else between them; at a run start the phrases
 * are tried in order, then the terms in order.  Every string is the reference's byte for byte, the same from run
 * to run.  A text with a byte >= 0x80 is not scanned: its items come back as SLG_HL_HOST (with Unicode, `\b` and
 * case folding depend on the regex crate's tables).
 *
 * SPECS.  Every query carries a list of field specs (spec_offsets [n_queries + 1] into specs).  A spec names the
 * text field and carries the FINAL word lists (the caller runs highlight_terms' analysis per field and
 * normalize_phrase_terms, as it analyses the input of slg_suggest_batch): word_offsets [n_terms + n_phrase_words +
 * 1] into word_bytes, the terms first, then the phrases' words; phrase_offsets [n_phrases + 1] counts the phrases'
 * words from 0.  Tags are any bytes and are copied verbatim.
 *
 * TWO ENTRY POINTS, one implementation.  slg_highlight_batch takes host hits in CSR per query (hit_offsets
 * [n_queries + 1] into hit_seg / hit_doc) against the index's current state.  slg_batch_highlight takes a
 * finished batch's own device rows (doc, seg, count of slg_batch_fetch) without a round trip: query q's hits are
 * its first count[q] rows, the state is the one the batch was prepared on, and any batch kind whose results are
 * those rows will do (the batch must have run; its sharded results are not read).  Both are synchronous.
 *
 * OUTPUT (slg_hl_out).  Items are query-major, then hit, then field spec in order.  status [n_items]:
 * SLG_HL_OK, SLG_HL_HOST (no fragments; highlight this one on the CPU), SLG_HL_NO_TEXT (the hit's segment has no
 * store for the field; no fragments).  offsets [n_items + 1]: item i's fragments are offsets[i] .. offsets[i + 1]
 * - 1; text_offsets [n_frags + 1] and text: fragment f is text[text_offsets[f] .. text_offsets[f + 1]), not
 * NUL-terminated.  item_capacity / frag_capacity = the entries status / text_offsets hold less the one more that
 * offsets / text_offsets need; text_capacity = the bytes of text.  The call fills n_items, n_frags and text_bytes.
 * SIZE QUERY: status, offsets, text_offsets and text all NULL: only the three totals are filled (the count pass
 * runs; nothing is emitted).
 *
 * SLG_ERR_INVALID: a NULL index, batch, out or array; a struct_size that is not the struct's; offsets that
 * decrease or do not start at 0; an unknown text field id; a host hit whose seg or doc is out of range; a term or
 * a phrase word of no bytes, a phrase of no words (the reference skips empty terms and phrases: drop them before
 * the call); some but not all of the four output arrays NULL; a capacity too small; a batch that has not run.
 * SLG_ERR_UNSUPPORTED (CPU path; the message names the query and the field spec): more than SLG_MAX_HL_TERMS terms,
 * SLG_MAX_HL_PHRASES phrases, SLG_MAX_PHRASE_TERMS words in a phrase, SLG_MAX_EXPAND_CHARS bytes in a word,
 * SLG_MAX_HL_TAG bytes in a tag, fragment_size above SLG_MAX_HL_FRAGMENT, number_of_fragments above
 * SLG_MAX_HL_FRAGMENTS, a word with a byte outside [0-9A-Za-z_], 2^32 or more bytes of output.  Never approximated.
 * NOT BUILT: non-ASCII texts and words (SLG_HL_HOST, or refused), analysis of the terms, `fields` /
 * return_stored, top_hits snippets through the aggregation fetch (pass their hits to slg_highlight_batch), the
 * sharded and coalesced paths, compressed doc-store decoding. */
#define SLG_MAX_HL_TERMS 32u
#define SLG_MAX_HL_PHRASES 8u
#define SLG_MAX_HL_TAG 64u         /* bytes of pre_tag and of post_tag */
#define SLG_MAX_HL_FRAGMENT 1024u  /* fragment_size */
#define SLG_MAX_HL_FRAGMENTS 8u    /* number_of_fragments */
enum { SLG_HL_OK = 0, SLG_HL_HOST = 1, SLG_HL_NO_TEXT = 2 };
typedef struct slg_hl_spec {
  uint32_t struct_size;            /* sizeof(slg_hl_spec) */
  int32_t text_field;              /* slg_index_add_text_field */
  uint32_t n_terms, n_phrases;
  const uint32_t *phrase_offsets;  /* [n_phrases + 1] over the phrases' words, from 0; NULL with n_phrases == 0 */
  const uint32_t *word_offsets;    /* [n_terms + phrase_offsets[n_phrases] + 1] into word_bytes, from 0 */
  const char *word_bytes;
  const char *pre_tag, *post_tag;
  uint32_t pre_len, post_len;
  uint32_t fragment_size, number_of_fragments;
} slg_hl_spec;
typedef struct slg_hl_out {
  uint32_t struct_size;            /* sizeof(slg_hl_out) */
  uint32_t item_capacity, frag_capacity;
  uint64_t text_capacity;
  uint8_t *status;                 /* [item_capacity] */
  uint32_t *offsets;               /* [item_capacity + 1] */
  uint32_t *text_offsets;          /* [frag_capacity + 1] */
  char *text;                      /* [text_capacity] */
  uint32_t n_items, n_frags;       /* filled by the call */
  uint64_t text_bytes;
} slg_hl_out;
int slg_index_add_text_field(slg_index *index, const uint64_t *const *seg_offsets, const uint8_t *const *seg_bytes);
int slg_index_remove_text_field(slg_index *index, int text_field_id);
int slg_highlight_batch(slg_index *index, uint32_t n_queries, const uint32_t *hit_offsets, const uint32_t *hit_seg,
                        const uint32_t *hit_doc, const uint32_t *spec_offsets, const slg_hl_spec *specs, slg_hl_out *out);
int slg_batch_highlight(slg_batch *batch, const uint32_t *spec_offsets, const slg_hl_spec *specs, slg_hl_out *out);
/* DIAGNOSTIC ONLY (tools/highlight_time.py): where the calling thread's last highlight call spent its time, in ms,
 * by the host clock: the count part (uploads, the count and scan kernels, the totals back, the wait) and the emit
 * part (the emit kernel, the strings back, the wait; 0 for a size query).  Per thread; `index` is only checked for
 * NULL; either pointer may be NULL. */
int slg_highlight_phase_ms(slg_index *index, double *count_ms, double *emit_ms);

/* ---------------------------------------------------------------------------------------------------------
 * explain (SearchRequest.explain): per returned hit the first-pass score, the value of every score function that
 * gave the doc one, the rescore part and the final score — HitExplanation (api/reader.rs:90-97), from
 * evaluate_compiled_score (:418-613), describe_function (:389-416), the score hook (:3038-3127), rescore_hits
 * (:3365-3383) and the final pass (:2803-2816).  A post-pass over a batch that has run, as slg_batch_highlight is:
 * no batch kind of its own, and a batch that is never explained runs what it runs without this call.
 *
 * slg_batch_explain explains the first min(rows, count[q]) rows of every query.  It is queued behind the batch's
 * last kernel on the batch's stream, works against the index state the batch was prepared on, and returns when the
 * caller's arrays are filled.  The arrays of slg_explain_out are the caller's, with a fixed stride of `rows` per
 * query (row r of query q at q * rows + r; entry e of that row at (q * rows + r) * SLG_MAX_EXPLAIN_FUNCS + e).
 * Rows at or beyond a query's count, and the entries behind a row's n_functions, are zero-filled.
 *
 * BASE SCORE.  base_score = ScorePlan::evaluate(leaves): the first-pass score of the row's doc before any score
 * stage.  The stages rewrite the candidates' scores in place, so it is computed again: the doc is looked up in every
 * posting list of the (query, row's segment) sub-query, with the batch's own term table (folded weights, leaves).
 * The arithmetic is the scoring kernels' for flat plans, every operation f32 and rounded on its own: impact *
 * weight per term; a leaf's terms added in query-term order from +0.0; Sum: the leaves added in leaf order from
 * -0.0; DisMax: max + tie * (sum - max), the sum from +0.0 over every leaf, the max from 0.0 when a leaf of the plan
 * has no term in the segment (else from -inf), a leaf without a posting of the doc counting as 0.0.
 *
 * FUNCTIONS.  The score stages run in the batch's order over that base, with the device functions the stages
 * themselves run.  A function_score appends, in request order, one entry per function that gives the doc a value:
 * a function whose filter rejects the doc appends nothing, neither does a decay without a value of the column, nor
 * a field_value_factor whose product or result is not finite.  fn_type is SLG_EXPLAIN_*, fn_field the agg field
 * id the caller named in f_field (-1 for a weight and for a script), fn_value the function's value as f32.  A
 * script_score appends one entry SLG_EXPLAIN_SCRIPT_SCORE with value script * boost.  Nesting follows
 * evaluate_compiled_score's recursion, inner entries first: SLG_SCRIPT_OUTER gives the function entries, then the
 * script entry; SLG_SCRIPT_INNER the script entry, then the function entries.  The substitution of 1.0 for a base
 * score within f32::EPSILON of 0 changes final_score, never the reported base_score.  A query without work in a
 * stage appends nothing for it.
 *
 * FINAL SCORE.  final_score is the end of the chain, computed again.  For every explained row of a batch without
 * rescore it is bit for bit the row's score as slg_batch_fetch returns it.
 *
 * RESCORE BATCH (legal only without score stages: n_functions is 0).  base_score is the first-pass score computed
 * again — first_score of slg_batch_fetch_rescore, bit for bit; rescored, rescore_score and combined_score are the
 * batch's own (rescored 0: the two scores are 0.0); final_score is the row's score: the combined score of a matched
 * row, the first-pass score of an unmatched row and of a row behind the window.  The three arrays are read only
 * for a rescore batch and must be given there; otherwise they may be NULL and are left alone.
 *
 * Errors.  SLG_ERR_INVALID, before any device work: a NULL batch, `out` or required array, rows == 0, a batch
 * that has not run, a batch whose index was destroyed.  SLG_ERR_UNSUPPORTED (CPU scorer), the reason named: rows >
 * SLG_MAX_EXPLAIN_ROWS, a scan batch, a hybrid batch, a batch with a two-level or deeper score plan, a query whose
 * term rows of all segments exceed 2048 entries (the kernel's LDS table), a batch whose last run was sharded.
 * Not built (CPU scorer): the inner hits of collapse, the hits of top_hits, scan batches (rank_feature entries),
 * vector-only results, the coalescer, and `profile`.
 * --------------------------------------------------------------------------------------------------------- */
#define SLG_MAX_EXPLAIN_ROWS 1024u /* rows of one query: 256 threads x 4 rows, as the rescore window */
#define SLG_MAX_EXPLAIN_FUNCS 9u   /* SLG_MAX_FSCORE_FUNCS + the script_score entry */
enum { SLG_EXPLAIN_WEIGHT = 0, SLG_EXPLAIN_FIELD_VALUE_FACTOR = 1, SLG_EXPLAIN_DECAY_EXP = 2,
       SLG_EXPLAIN_DECAY_GAUSS = 3, SLG_EXPLAIN_DECAY_LINEAR = 4, SLG_EXPLAIN_SCRIPT_SCORE = 5 };
typedef struct slg_explain_out {
  float *base_score;      /* [nq * rows] */
  float *final_score;     /* [nq * rows] */
  uint32_t *n_functions;  /* [nq * rows] entries of the row, <= SLG_MAX_EXPLAIN_FUNCS */
  uint32_t *fn_type;      /* [nq * rows * SLG_MAX_EXPLAIN_FUNCS] SLG_EXPLAIN_* */
  int32_t *fn_field;      /* [nq * rows * SLG_MAX_EXPLAIN_FUNCS] agg field id, or -1 */
  float *fn_value;        /* [nq * rows * SLG_MAX_EXPLAIN_FUNCS] */
  uint32_t *rescored;     /* [nq * rows]; a rescore batch only, else NULL or left alone */
  float *rescore_score;   /* [nq * rows]; as rescored */
  float *combined_score;  /* [nq * rows]; as rescored */
} slg_explain_out;
int slg_batch_explain(slg_batch *batch, uint32_t rows, const slg_explain_out *out);

#ifdef __cplusplus
}
#endif
#endif /* SEARCHLITE_GPU_H */
