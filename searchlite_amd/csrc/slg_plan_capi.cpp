// slg_plan_capi.cpp — a small C ABI over the host planner (slg_plan.cpp) for the CPU unit tests
// (tests/test_plan.py) and the CPU sanitizer run (tools/sanitize_cpu.sh): the planner is pure host
// code, so its invariants are checked without a GPU.  Built as lib/libslg_plan.so with g++; NOT
// part of libsearchlite_gpu.so's exported surface (the product calls slgplan::plan_batch directly).
#include <cstring>
#include <new>

#include "slg_date.hpp"
#include "slg_plan.hpp"

extern "C" {

struct slgp_segment {
  uint32_t n_docs, n_terms;
  const uint64_t *term_offsets;
  const float *champ;  // [n_terms * 68] or NULL
};

struct slgp_facts {
  uint64_t n_postings, n_postings_essential, n_postings_nonessential, n_rounds, n_bounds, n_bnd, cand_total;
  uint64_t image_bytes;
  uint32_t n_sq, n_terms, n_slices, max_terms;
  uint32_t uniform, multi, plan_batch, nested, pruned, cand_mode;
  uint32_t sizeof_round_query, sizeof_term_ref;
  uint32_t deep;
};

// -> opaque plan or NULL (err / code filled)
void *slgp_plan(const slgp_segment *segs, uint32_t n_segs, const slg_tuning *tuning, uint32_t nq,
                const uint32_t *q_offsets, const uint32_t *q_term_ids, const float *q_weights,
                const slg_score_plans *plans, const int32_t *q_filter, uint32_t k, int strategy,
                const char *filter_live, uint32_t n_filters, char *err, uint32_t err_len, int *code) {
  try {
    std::vector<slgplan::SegView> views(n_segs);
    for (uint32_t s = 0; s < n_segs; s++) {
      views[s].n_docs = segs[s].n_docs;
      views[s].n_terms = segs[s].n_terms;
      views[s].term_offsets = segs[s].term_offsets;
      views[s].champ = segs[s].champ;
    }
    slgplan::BatchIn in;
    in.nq = nq;
    in.q_offsets = q_offsets;
    in.q_term_ids = q_term_ids;
    in.q_weights = q_weights;
    if (plans) in.plans = *plans;
    in.q_filter = q_filter;
    in.k = k;
    in.strategy = strategy;
    in.filter_live = filter_live;
    in.n_filters = n_filters;
    auto *p = new slgplan::Plan();
    try {
      slgplan::plan_batch(views, *tuning, in, *p);
    } catch (...) {
      delete p;
      throw;
    }
    if (code) *code = SLG_OK;
    return p;
  } catch (const slgplan::SlgError &e) {
    if (err && err_len) {
      std::strncpy(err, e.what(), err_len - 1);
      err[err_len - 1] = 0;
    }
    if (code) *code = e.code;
  } catch (const std::exception &e) {
    if (err && err_len) {
      std::strncpy(err, e.what(), err_len - 1);
      err[err_len - 1] = 0;
    }
    if (code) *code = SLG_ERR_INTERNAL;
  }
  return nullptr;
}

void slgp_facts_of(const void *plan, slgp_facts *f) {
  const auto &p = *static_cast<const slgplan::Plan *>(plan);
  f->n_postings = p.n_postings;
  f->n_postings_essential = p.n_postings_essential;
  f->n_postings_nonessential = p.n_postings_nonessential;
  f->n_rounds = p.n_rounds;
  f->n_bounds = p.n_bounds;
  f->n_bnd = p.n_bnd;
  f->cand_total = p.cand_total;
  f->image_bytes = p.image_bytes;
  f->n_sq = (uint32_t)p.sqs.size();
  f->n_terms = (uint32_t)p.terms.size();
  f->n_slices = (uint32_t)p.slice_sq.size();
  f->max_terms = p.max_terms;
  f->uniform = p.uniform;
  f->multi = p.multi;
  f->plan_batch = p.plan_batch;
  f->nested = p.nested;
  f->pruned = p.pruned;
  f->cand_mode = p.cand_mode;
  f->sizeof_round_query = (uint32_t)sizeof(slg::RoundQuery);
  f->sizeof_term_ref = (uint32_t)sizeof(slg::TermRef);
  f->deep = p.deep;
}

// what: 0 sub-queries (RoundQuery), 1 terms (TermRef), 2 slice_sq, 3 slice_seg, 4 slice_order,
// 5 query refs (2 x u32), 6 bnd_coarse, 7 q_postings (u64), 8 the packed image, 9 deep-tree nodes (PlanNode)
uint64_t slgp_bytes(const void *plan, int what) {
  const auto &p = *static_cast<const slgplan::Plan *>(plan);
  switch (what) {
    case 0: return p.sqs.size() * sizeof(slg::RoundQuery);
    case 1: return p.terms.size() * sizeof(slg::TermRef);
    case 2: return p.slice_sq.size() * 4;
    case 3: return p.slice_seg.size() * 4;
    case 4: return p.slice_order.size() * 4;
    case 5: return p.qrefs.size() * sizeof(slg::QueryRef);
    case 6: return p.bnd_coarse.size() * 4;
    case 7: return p.q_postings.size() * 8;
    case 8: return p.image_bytes;
    case 9: return p.nodes.size() * sizeof(slg::PlanNode);
  }
  return 0;
}

void slgp_copy(const void *plan, int what, void *dst) {
  const auto &p = *static_cast<const slgplan::Plan *>(plan);
  const void *src = nullptr;
  switch (what) {
    case 0: src = p.sqs.data(); break;
    case 1: src = p.terms.data(); break;
    case 2: src = p.slice_sq.data(); break;
    case 3: src = p.slice_seg.data(); break;
    case 4: src = p.slice_order.data(); break;
    case 5: src = p.qrefs.data(); break;
    case 6: src = p.bnd_coarse.data(); break;
    case 7: src = p.q_postings.data(); break;
    case 8: p.pack(static_cast<unsigned char *>(dst)); return;
    case 9: src = p.nodes.data(); break;
  }
  const uint64_t n = slgp_bytes(plan, what);
  if (n && src) std::memcpy(dst, src, n);
}

void slgp_free(void *plan) { delete static_cast<slgplan::Plan *>(plan); }

// the host side of slg_index_add_sort_field_i64 / _f64 (kind 1 / 2) for one segment: per doc the ascending
// and descending u64 keys and the presence bitmap ((n_docs + 31) / 32 words).  0, or a negative error code
int slgp_sort_keys(int kind, uint32_t n_docs, const uint32_t *offsets, const void *values, uint64_t *asc,
                   uint64_t *desc, uint32_t *present_words) {
  try {
    slgplan::sort_field_keys(kind, n_docs, offsets, values, asc, desc, present_words);
    return SLG_OK;
  } catch (const slgplan::SlgError &e) {
    return e.code;
  }
}

// the host side of slg_batch_prepare_after: the select kernels' key words of one cursor (slgplan::cursor_key;
// n_parts 0 = score order, 3 words; else kind[p] 0 `_score` / 1 i64 / 2 f64, 14 words).  0, or a negative
// error code
int slgp_cursor_key(uint32_t n_parts, const int *kind, const int32_t *order, const slg_sort_cursor *cursor,
                    uint32_t *out_words) {
  try {
    if (!cursor || !out_words || (n_parts && (!kind || !order))) return SLG_ERR_INVALID;
    slgplan::cursor_key(n_parts, kind, order, *cursor, out_words);
    return SLG_OK;
  } catch (const slgplan::SlgError &e) {
    return e.code;
  }
}

// the host side of slg_batch_prepare_bool: check_bool, then plan_bool against the segments.  queries: nq x 8
// words (slg::BoolQuery); terms: room for terms_cap entries of 4 words (slg::BoolTerm: off low, off high, df,
// group), filled when the tables fit; *n_terms: the entries the tables have.  0, or a negative error code (err filled)
int slgp_plan_bool(const slgp_segment *segs, uint32_t n_segs, uint32_t nq, const slg_bool_spec *spec,
                   const slg_score_plans *plans, uint32_t *queries, uint32_t *terms, uint32_t terms_cap,
                   uint32_t *n_terms, char *err, uint32_t err_len) {
  try {
    slgplan::check_bool(spec, nq, plans);
    std::vector<slgplan::SegView> views(n_segs);
    for (uint32_t s = 0; s < n_segs; s++) {
      views[s].n_docs = segs[s].n_docs;
      views[s].n_terms = segs[s].n_terms;
      views[s].term_offsets = segs[s].term_offsets;
    }
    slgplan::BoolPlan bp;
    slgplan::plan_bool(views, nq, *spec, bp);
    static_assert(sizeof(slg::BoolQuery) == 32 && sizeof(slg::BoolTerm) == 16, "the words the caller reads");
    if (queries && nq) std::memcpy(queries, bp.queries.data(), (size_t)nq * sizeof(slg::BoolQuery));
    if (n_terms) *n_terms = (uint32_t)bp.terms.size();
    if (terms && bp.terms.size() <= terms_cap && !bp.terms.empty())
      std::memcpy(terms, bp.terms.data(), bp.terms.size() * sizeof(slg::BoolTerm));
    return SLG_OK;
  } catch (const slgplan::SlgError &e) {
    if (err && err_len) {
      std::strncpy(err, e.what(), err_len - 1);
      err[err_len - 1] = 0;
    }
    return e.code;
  }
}

// the host side of slg_batch_prepare_bool_tree: check_bool_tree, then plan_bool_tree against the segments and
// filters that exist as descriptions only (reject bitmaps: the addresses slgp_plan_fscore makes up, (f + 1) << 32 |
// s << 8 | 3).  queries: nq x 8 words (slg::BoolTreeQuery); nodes: entries of 8 words (slg::BoolTreeNode: must,
// must_not, should as low / high words, min_should, pad); terms: entries of 4 words (slg::BoolTerm); filters:
// addresses; filt_rows: words.  Each table is filled when it fits its cap; counts: entries of nodes, terms,
// filters, filt_rows.  0, or a negative error code (err filled)
int slgp_plan_bool_tree(const slgp_segment *segs, uint32_t n_segs, const char *filter_live, uint32_t n_filters,
                        uint32_t nq, const slg_bool_tree_spec *spec, const slg_score_plans *plans, uint32_t *queries,
                        uint32_t *nodes, uint32_t nodes_cap, uint32_t *terms, uint32_t terms_cap, uint64_t *filters,
                        uint32_t filters_cap, uint32_t *filt_rows, uint32_t filt_rows_cap, uint32_t *counts,
                        char *err, uint32_t err_len) {
  try {
    slgplan::check_bool_tree(spec, nq, plans);
    std::vector<slgplan::SegView> views(n_segs);
    for (uint32_t s = 0; s < n_segs; s++) {
      views[s].n_docs = segs[s].n_docs;
      views[s].n_terms = segs[s].n_terms;
      views[s].term_offsets = segs[s].term_offsets;
    }
    std::vector<const uint32_t *> reject((size_t)n_filters * n_segs);
    for (uint32_t f = 0; f < n_filters; f++)
      for (uint32_t s = 0; s < n_segs; s++)
        reject[(size_t)f * n_segs + s] =
            reinterpret_cast<const uint32_t *>((uintptr_t)(((uint64_t)(f + 1) << 32) | ((uint64_t)s << 8) | 3u));
    slgplan::BoolTreePlan tp;
    slgplan::plan_bool_tree(views, reject.data(), filter_live, n_filters, nq, *spec, tp);
    static_assert(sizeof(slg::BoolTreeQuery) == 32 && sizeof(slg::BoolTreeNode) == 32 && sizeof(slg::BoolTerm) == 16,
                  "the words the caller reads");
    if (queries && nq) std::memcpy(queries, tp.queries.data(), (size_t)nq * sizeof(slg::BoolTreeQuery));
    if (nodes && tp.nodes.size() <= nodes_cap && !tp.nodes.empty())
      std::memcpy(nodes, tp.nodes.data(), tp.nodes.size() * sizeof(slg::BoolTreeNode));
    if (terms && tp.terms.size() <= terms_cap && !tp.terms.empty())
      std::memcpy(terms, tp.terms.data(), tp.terms.size() * sizeof(slg::BoolTerm));
    if (filters && tp.filters.size() <= filters_cap && !tp.filters.empty())
      std::memcpy(filters, tp.filters.data(), tp.filters.size() * sizeof(void *));
    if (filt_rows && tp.filt_rows.size() <= filt_rows_cap && !tp.filt_rows.empty())
      std::memcpy(filt_rows, tp.filt_rows.data(), tp.filt_rows.size() * 4);
    if (counts) {
      counts[0] = (uint32_t)tp.nodes.size();
      counts[1] = (uint32_t)tp.terms.size();
      counts[2] = (uint32_t)tp.filters.size();
      counts[3] = (uint32_t)tp.filt_rows.size();
    }
    return SLG_OK;
  } catch (const slgplan::SlgError &e) {
    if (err && err_len) {
      std::strncpy(err, e.what(), err_len - 1);
      err[err_len - 1] = 0;
    }
    return e.code;
  }
}

// the three-valued pass booltree_filter_kernel runs after every step of a row (slg::booltree_eval, slg_desc.hpp):
// nodes: n_nodes entries of 8 words as slgp_plan_bool_tree writes them; *t / *f: the values known to be true /
// false going in (leaf bits), with the decided nodes' bits added coming out
void slgp_booltree_eval(const uint32_t *nodes, uint32_t n_nodes, uint64_t *t, uint64_t *f) {
  const auto node_at = [nodes](uint32_t i) {
    slg::BoolTreeNode n;
    std::memcpy(&n, nodes + (size_t)i * 8, sizeof n);
    return n;
  };
  slg::booltree_eval(node_at, n_nodes, *t, *f);
}

// the host side of slg_batch_prepare_phrase: check_phrase, then plan_phrase against the segments.  seg_has_pos:
// one byte per segment, 0 = no positions were set for it (NULL: every segment has positions).  queries: nq x 8
// words (slg::BoolQuery); pqueries: nq x 8 words (slg::PhraseQuery); vars: entries of 4 words (slg::PhraseVar);
// terms: entries of 6 words (slg::PhraseTerm: off low, off high, ubase low, ubase high, df, pad); bterms: entries
// of 4 words (slg::BoolTerm).  Each table is filled when it fits its cap; counts: its entries (vars, terms,
// bterms).  0, or a negative error code (err filled)
int slgp_plan_phrase(const slgp_segment *segs, const uint8_t *seg_has_pos, uint32_t n_segs, uint32_t nq,
                     const slg_bool_spec *boolean, const slg_phrase_spec *spec, const slg_score_plans *plans,
                     uint32_t *queries, uint32_t *pqueries, uint32_t *vars, uint32_t vars_cap, uint32_t *terms,
                     uint32_t terms_cap, uint32_t *bterms, uint32_t bterms_cap, uint32_t *counts, char *err,
                     uint32_t err_len) {
  try {
    slgplan::check_phrase(boolean, spec, nq, plans);
    std::vector<slgplan::SegView> views(n_segs);
    for (uint32_t s = 0; s < n_segs; s++) {
      views[s].n_docs = segs[s].n_docs;
      views[s].n_terms = segs[s].n_terms;
      views[s].term_offsets = segs[s].term_offsets;
      views[s].has_positions = seg_has_pos ? seg_has_pos[s] != 0 : true;
    }
    slgplan::PhrasePlan pp;
    slgplan::plan_phrase(views, nq, boolean, *spec, pp);
    static_assert(sizeof(slg::PhraseQuery) == 32 && sizeof(slg::PhraseVar) == 16 && sizeof(slg::PhraseTerm) == 24,
                  "the words the caller reads");
    if (queries && nq) std::memcpy(queries, pp.bools.queries.data(), (size_t)nq * sizeof(slg::BoolQuery));
    if (pqueries && nq) std::memcpy(pqueries, pp.queries.data(), (size_t)nq * sizeof(slg::PhraseQuery));
    if (vars && pp.vars.size() <= vars_cap && !pp.vars.empty())
      std::memcpy(vars, pp.vars.data(), pp.vars.size() * sizeof(slg::PhraseVar));
    if (terms && pp.terms.size() <= terms_cap && !pp.terms.empty())
      std::memcpy(terms, pp.terms.data(), pp.terms.size() * sizeof(slg::PhraseTerm));
    if (bterms && pp.bools.terms.size() <= bterms_cap && !pp.bools.terms.empty())
      std::memcpy(bterms, pp.bools.terms.data(), pp.bools.terms.size() * sizeof(slg::BoolTerm));
    if (counts) {
      counts[0] = (uint32_t)pp.vars.size();
      counts[1] = (uint32_t)pp.terms.size();
      counts[2] = (uint32_t)pp.bools.terms.size();
    }
    return SLG_OK;
  } catch (const slgplan::SlgError &e) {
    if (err && err_len) {
      std::strncpy(err, e.what(), err_len - 1);
      err[err_len - 1] = 0;
    }
    return e.code;
  }
}

// the host side of slg_batch_prepare_fscore: check_fscore, then plan_fscore against registered fields and filters
// that exist as descriptions only.  A field's column of segment s: seg_has[s] 0 = none; seg_dense[s] 1 = stored
// without offsets.  The tables carry addresses that are never read and name what they stand for: a column's values
// (id + 1) << 32 | s << 8 | 1, its offsets the same | 2 (0 when dense), the reject bitmap of filter f in segment s
// (f + 1) << 32 | s << 8 | 3.  queries: nq x 8 words (slg::FscoreQuery); fns: entries of 16 words (slg::FscoreFn);
// cols: entries of two addresses (offsets, values); filters: addresses.  Each table is filled when it fits its cap;
// counts: entries of fns, cols, filters, then the queries with work and 1 for the full kernel.  0, or a negative
// error code (err filled)
struct slgp_fscore_field {
  int32_t id;
  uint32_t keyword, non_finite;
  const uint8_t *seg_has, *seg_dense;
};
}  // extern "C"
// the view of a described field (slgp_fscore_field, slgp_filter_field): its id, kind and made-up column addresses
template <typename F>
static slgplan::FscoreFieldView described_field(const F &f, uint32_t n_segs) {
  slgplan::FscoreFieldView v;
  v.id = f.id;
  v.keyword = f.keyword != 0;
  v.per_seg.assign(n_segs, slg::ColumnDev{nullptr, nullptr});
  for (uint32_t s = 0; s < n_segs; s++) {
    if (!f.seg_has[s]) continue;
    const uint64_t a = ((uint64_t)(f.id + 1) << 32) | ((uint64_t)s << 8);
    v.per_seg[s].vals = reinterpret_cast<const void *>((uintptr_t)(a | 1u));
    if (!f.seg_dense[s]) v.per_seg[s].offs = reinterpret_cast<const uint32_t *>((uintptr_t)(a | 2u));
  }
  return v;
}
extern "C" {
int slgp_plan_fscore(const slgp_fscore_field *fields, uint32_t n_fields, const char *filter_live, uint32_t n_filters,
                     uint32_t n_segs, uint32_t nq, const slg_fscore_spec *spec, uint32_t *queries, uint32_t *fns,
                     uint32_t fns_cap, uint64_t *cols, uint32_t cols_cap, uint64_t *filters, uint32_t filters_cap,
                     uint32_t *counts, char *err, uint32_t err_len) {
  try {
    slgplan::check_fscore(spec, nq);
    std::vector<slgplan::FscoreFieldView> views(n_fields);
    for (uint32_t i = 0; i < n_fields; i++) {
      views[i] = described_field(fields[i], n_segs);
      views[i].non_finite = fields[i].non_finite != 0;
    }
    std::vector<const uint32_t *> reject((size_t)n_filters * n_segs);
    for (uint32_t f = 0; f < n_filters; f++)
      for (uint32_t s = 0; s < n_segs; s++)
        reject[(size_t)f * n_segs + s] =
            reinterpret_cast<const uint32_t *>((uintptr_t)(((uint64_t)(f + 1) << 32) | ((uint64_t)s << 8) | 3u));
    slgplan::FscorePlan fp;
    slgplan::plan_fscore(views, reject.data(), filter_live, n_filters, n_segs, nq, *spec, fp);
    static_assert(sizeof(slg::FscoreQuery) == 32 && sizeof(slg::FscoreFn) == 64 && sizeof(slg::ColumnDev) == 16,
                  "the words the caller reads");
    if (queries && nq) std::memcpy(queries, fp.queries.data(), (size_t)nq * sizeof(slg::FscoreQuery));
    if (fns && fp.fns.size() <= fns_cap && !fp.fns.empty())
      std::memcpy(fns, fp.fns.data(), fp.fns.size() * sizeof(slg::FscoreFn));
    if (cols && fp.cols.size() <= cols_cap && !fp.cols.empty())
      std::memcpy(cols, fp.cols.data(), fp.cols.size() * sizeof(slg::ColumnDev));
    if (filters && fp.filters.size() <= filters_cap && !fp.filters.empty())
      std::memcpy(filters, fp.filters.data(), fp.filters.size() * sizeof(void *));
    if (counts) {
      counts[0] = (uint32_t)fp.fns.size();
      counts[1] = (uint32_t)fp.cols.size();
      counts[2] = (uint32_t)fp.filters.size();
      counts[3] = fp.n_work;
      counts[4] = fp.full ? 1u : 0u;
    }
    return SLG_OK;
  } catch (const slgplan::SlgError &e) {
    if (err && err_len) {
      std::strncpy(err, e.what(), err_len - 1);
      err[err_len - 1] = 0;
    }
    return e.code;
  }
}

// the host side of slg_batch_prepare_scan: check_scan, then plan_scan against segments of seg_docs[s] docs and
// registered fields and filters that exist as descriptions only (slgp_fscore_field, the made-up addresses of
// slgp_plan_fscore).  full_regions: the batch has a sort spec or aggregations.  queries: nq x 8 words
// (slg::ScanQuery); qrefs: nq x 2 words; slices: entries of 8 words (slg::ScanSlice: q, seg, first_doc, n_docs, cap,
// pad); cbeg: the regions' first entries; cols: entries of two addresses (offsets, values); root: nq words (0 = none,
// f + 1; zeros when no query has a root filter).  slices, cbeg and cols are filled when they fit their cap; counts:
// entries of slices and cols, 1 for the full kernel, then cand_total's low and high word.  0, or a negative error
// code (err filled).  slgp_scan_slice_docs: the docs per slice the planner cuts at
uint32_t slgp_scan_slice_docs(void) { return slg::kScanSliceDocs; }
int slgp_plan_scan(const uint32_t *seg_docs, uint32_t n_segs, const slgp_fscore_field *fields, uint32_t n_fields,
                   const char *filter_live, uint32_t n_filters, uint32_t nq, const slg_scan_spec *spec,
                   const int32_t *q_filter, uint32_t full_regions, uint32_t k, uint32_t *queries, uint32_t *qrefs,
                   uint32_t *slices, uint64_t *cbeg, uint32_t slices_cap, uint64_t *cols, uint32_t cols_cap,
                   uint32_t *root, uint32_t *counts, char *err, uint32_t err_len) {
  try {
    slgplan::check_scan(spec, nq, k);
    if (n_segs && !seg_docs) throw slgplan::SlgError(SLG_ERR_INVALID, "seg_docs is NULL");
    std::vector<slgplan::FscoreFieldView> views(n_fields);
    for (uint32_t i = 0; i < n_fields; i++) {
      views[i] = described_field(fields[i], n_segs);
      views[i].non_finite = fields[i].non_finite != 0;
    }
    slgplan::ScanPlan sp;
    slgplan::plan_scan(std::vector<uint32_t>(seg_docs, seg_docs + n_segs), views, filter_live, n_filters, nq, *spec,
                       q_filter, full_regions != 0, k, sp);
    static_assert(sizeof(slg::ScanQuery) == 32 && sizeof(slg::ScanSlice) == 32 && sizeof(slg::QueryRef) == 8,
                  "the words the caller reads");
    if (queries && nq) std::memcpy(queries, sp.queries.data(), (size_t)nq * sizeof(slg::ScanQuery));
    if (qrefs && nq) std::memcpy(qrefs, sp.qrefs.data(), (size_t)nq * sizeof(slg::QueryRef));
    if (sp.slices.size() <= slices_cap && !sp.slices.empty()) {
      if (slices) std::memcpy(slices, sp.slices.data(), sp.slices.size() * sizeof(slg::ScanSlice));
      if (cbeg) std::memcpy(cbeg, sp.slice_cbeg.data(), sp.slice_cbeg.size() * 8);
    }
    if (cols && sp.cols.size() <= cols_cap && !sp.cols.empty())
      std::memcpy(cols, sp.cols.data(), sp.cols.size() * sizeof(slg::ColumnDev));
    if (root && nq) {
      std::memset(root, 0, (size_t)nq * 4);
      if (!sp.q_filter.empty()) std::memcpy(root, sp.q_filter.data(), (size_t)nq * 4);
    }
    if (counts) {
      counts[0] = (uint32_t)sp.slices.size();
      counts[1] = (uint32_t)sp.cols.size();
      counts[2] = sp.full ? 1u : 0u;
      counts[3] = (uint32_t)sp.cand_total;
      counts[4] = (uint32_t)(sp.cand_total >> 32);
    }
    return SLG_OK;
  } catch (const slgplan::SlgError &e) {
    if (err && err_len) {
      std::strncpy(err, e.what(), err_len - 1);
      err[err_len - 1] = 0;
    }
    return e.code;
  }
}

// the host side of slg_batch_prepare_script: check_script_order and check_script, then plan_script against
// registered fields that exist as descriptions only (slgp_fscore_field, the made-up addresses of slgp_plan_fscore).
// queries: nq x 16 words (slg::ScriptQuery); instrs: entries of 4 words (slg::ScriptInstr); cols: entries of two
// addresses (offsets, values).  Each table is filled when it fits its cap; counts: entries of instrs and cols, then
// the queries with a program and the batch's deepest stack.  0, or a negative error code (err filled)
int slgp_plan_script(const slgp_fscore_field *fields, uint32_t n_fields, uint32_t n_segs, uint32_t nq,
                     const slg_script_spec *spec, int order, uint32_t *queries, uint32_t *instrs, uint32_t instrs_cap,
                     uint64_t *cols, uint32_t cols_cap, uint32_t *counts, char *err, uint32_t err_len) {
  try {
    slgplan::ScriptShape shape;
    slgplan::check_script_order(order);  // (an invalid argument comes before an unsupported program)
    slgplan::check_script(spec, nq, shape);
    std::vector<slgplan::FscoreFieldView> views(n_fields);
    for (uint32_t i = 0; i < n_fields; i++) {
      views[i] = described_field(fields[i], n_segs);
      views[i].non_finite = fields[i].non_finite != 0;
    }
    slgplan::ScriptPlan sp;
    slgplan::plan_script(views, n_segs, nq, *spec, shape, sp);
    static_assert(sizeof(slg::ScriptQuery) == 64 && sizeof(slg::ScriptInstr) == 16 && sizeof(slg::ColumnDev) == 16,
                  "the words the caller reads");
    if (queries && nq) std::memcpy(queries, sp.queries.data(), (size_t)nq * sizeof(slg::ScriptQuery));
    if (instrs && sp.instrs.size() <= instrs_cap && !sp.instrs.empty())
      std::memcpy(instrs, sp.instrs.data(), sp.instrs.size() * sizeof(slg::ScriptInstr));
    if (cols && sp.cols.size() <= cols_cap && !sp.cols.empty())
      std::memcpy(cols, sp.cols.data(), sp.cols.size() * sizeof(slg::ColumnDev));
    if (counts) {
      counts[0] = (uint32_t)sp.instrs.size();
      counts[1] = (uint32_t)sp.cols.size();
      counts[2] = sp.n_work;
      counts[3] = sp.max_depth;
    }
    return SLG_OK;
  } catch (const slgplan::SlgError &e) {
    if (err && err_len) {
      std::strncpy(err, e.what(), err_len - 1);
      err[err_len - 1] = 0;
    }
    return e.code;
  }
}

// the host side of slg_index_add_filter_trees: check_filter_trees, then plan_filter_trees against registered fields
// and filters that exist as descriptions only (columns and reject bitmaps: the addresses slgp_plan_fscore makes
// up; a filter with filter_live 0 has none).  tree_rows: n_trees x 2 words (slg::FilterTreeDev); nodes: entries of
// 8 words (slg::FilterNodeDev); cols: entries of two addresses (offsets, values); filters: addresses; words: the
// ordinal bit sets.  Each table is filled when it fits its cap; counts: entries of nodes, cols, filters, words.
// 0, or a negative error code (err filled)
struct slgp_filter_field {
  int32_t id;
  uint32_t keyword, n_ords, from_i64, any_value;
  double vmin, vmax;
  const uint8_t *seg_has, *seg_dense;
};
int slgp_plan_filter_trees(const slgp_filter_field *fields, uint32_t n_fields, const char *filter_live,
                           uint32_t n_filters, uint32_t n_segs, const slg_filter_tree *trees, uint32_t n_trees,
                           uint32_t *tree_rows, uint32_t *nodes, uint32_t nodes_cap, uint64_t *cols, uint32_t cols_cap,
                           uint64_t *filters, uint32_t filters_cap, uint32_t *words, uint32_t words_cap,
                           uint32_t *counts, char *err, uint32_t err_len) {
  try {
    slgplan::check_filter_trees(trees, n_trees);
    std::vector<slgplan::FscoreFieldView> views(n_fields);
    for (uint32_t i = 0; i < n_fields; i++) {
      views[i] = described_field(fields[i], n_segs);
      views[i].n_ords = fields[i].n_ords;
      views[i].from_i64 = fields[i].from_i64 != 0;
      views[i].any_value = fields[i].any_value != 0;
      views[i].vmin = fields[i].vmin;
      views[i].vmax = fields[i].vmax;
    }
    std::vector<const uint32_t *> reject((size_t)n_filters * n_segs, nullptr);
    for (uint32_t f = 0; f < n_filters; f++)
      for (uint32_t s = 0; s < n_segs && filter_live[f]; s++)
        reject[(size_t)f * n_segs + s] =
            reinterpret_cast<const uint32_t *>((uintptr_t)(((uint64_t)(f + 1) << 32) | ((uint64_t)s << 8) | 3u));
    slgplan::FilterTreePlan fp;
    slgplan::plan_filter_trees(views, reject.data(), filter_live, n_filters, n_segs, trees, n_trees, fp);
    static_assert(sizeof(slg::FilterTreeDev) == 8 && sizeof(slg::FilterNodeDev) == 32, "the words the caller reads");
    if (tree_rows) std::memcpy(tree_rows, fp.trees.data(), fp.trees.size() * sizeof(slg::FilterTreeDev));
    if (nodes && fp.nodes.size() <= nodes_cap) std::memcpy(nodes, fp.nodes.data(), fp.nodes.size() * sizeof(slg::FilterNodeDev));
    if (cols && fp.cols.size() <= cols_cap && !fp.cols.empty())
      std::memcpy(cols, fp.cols.data(), fp.cols.size() * sizeof(slg::ColumnDev));
    if (filters && fp.filters.size() <= filters_cap && !fp.filters.empty())
      std::memcpy(filters, fp.filters.data(), fp.filters.size() * sizeof(void *));
    if (words && fp.words.size() <= words_cap && !fp.words.empty())
      std::memcpy(words, fp.words.data(), fp.words.size() * 4);
    if (counts) {
      counts[0] = (uint32_t)fp.nodes.size();
      counts[1] = (uint32_t)fp.cols.size();
      counts[2] = (uint32_t)fp.filters.size();
      counts[3] = (uint32_t)fp.words.size();
    }
    return SLG_OK;
  } catch (const slgplan::SlgError &e) {
    if (err && err_len) {
      std::strncpy(err, e.what(), err_len - 1);
      err[err_len - 1] = 0;
    }
    return e.code;
  }
}

// the host side of slg_index_add_nested_filter_trees: check_nested_filter_trees, then plan_nested_filter_trees
// against agg fields and filters described as above and nested paths and nested fields that exist as descriptions
// only (their arrays: made-up addresses, owner id + 1 in the high word, the segment, a tag).  scope_rows: entries
// of 4 words (slg::NestedScopeDev); nodes: entries of 8 words; levels: level_begin; words: the ordinal bit sets.
// Each table is filled when it fits its cap; counts: entries of scope_rows, nodes, levels, words, then the rows of
// the path table and of the nested column table.  0, or a negative error code (err filled)
struct slgp_nested_path {
  int32_t id, parent;
  const uint8_t *seg_has;
};
struct slgp_nested_field {
  int32_t id, path;
  uint32_t kind, n_ords;  // kind: 1 f64, 2 i64, 3 keyword ordinals
  const uint8_t *seg_has;
};
int slgp_plan_nested_filter_trees(const slgp_filter_field *fields, uint32_t n_fields, const char *filter_live,
                                  uint32_t n_filters, const slgp_nested_path *paths, uint32_t n_paths,
                                  const slgp_nested_field *nested_fields, uint32_t n_nested_fields, uint32_t n_segs,
                                  const slg_nested_filter_tree *trees, uint32_t n_trees, uint32_t *scope_rows,
                                  uint32_t scopes_cap, uint32_t *nodes, uint32_t nodes_cap, uint32_t *levels,
                                  uint32_t levels_cap, uint32_t *words, uint32_t words_cap, uint32_t *counts, char *err,
                                  uint32_t err_len) {
  try {
    slgplan::check_nested_filter_trees(trees, n_trees);
    std::vector<slgplan::FscoreFieldView> views(n_fields);
    for (uint32_t i = 0; i < n_fields; i++) {
      views[i] = described_field(fields[i], n_segs);
      views[i].n_ords = fields[i].n_ords;
      views[i].from_i64 = fields[i].from_i64 != 0;
      views[i].any_value = fields[i].any_value != 0;
      views[i].vmin = fields[i].vmin;
      views[i].vmax = fields[i].vmax;
    }
    std::vector<const uint32_t *> reject((size_t)n_filters * n_segs, nullptr);
    for (uint32_t f = 0; f < n_filters; f++)
      for (uint32_t s = 0; s < n_segs && filter_live[f]; s++)
        reject[(size_t)f * n_segs + s] =
            reinterpret_cast<const uint32_t *>((uintptr_t)(((uint64_t)(f + 1) << 32) | ((uint64_t)s << 8) | 3u));
    const auto made_up = [](int32_t owner, uint32_t s, uint32_t tag) {
      return reinterpret_cast<const uint32_t *>((uintptr_t)(((uint64_t)(owner + 1) << 32) | ((uint64_t)s << 8) | tag));
    };
    std::vector<slgplan::NestedPathView> pviews(n_paths);
    for (uint32_t i = 0; i < n_paths; i++) {
      pviews[i].id = paths[i].id;
      pviews[i].parent = paths[i].parent;
      pviews[i].per_seg.assign(n_segs, slg::NestedPathDev{});
      for (uint32_t s = 0; s < n_segs; s++)
        if (paths[i].seg_has[s])
          pviews[i].per_seg[s] = slg::NestedPathDev{made_up(paths[i].id, s, 4u), made_up(paths[i].id, s, 5u),
                                                    made_up(paths[i].id, s, 6u), made_up(paths[i].id, s, 7u), 0u, 0u};
    }
    std::vector<slgplan::NestedFieldView> nviews(n_nested_fields);
    for (uint32_t i = 0; i < n_nested_fields; i++) {
      const slgp_nested_field &f = nested_fields[i];
      nviews[i].id = f.id;
      nviews[i].path = f.path;
      nviews[i].kind = (int)f.kind;
      nviews[i].n_ords = f.n_ords;
      nviews[i].per_seg.assign(n_segs, slg::NestedColDev{});
      nviews[i].has.assign(f.seg_has, f.seg_has + n_segs);
      for (uint32_t s = 0; s < n_segs; s++)
        if (f.seg_has[s]) nviews[i].per_seg[s] = slg::NestedColDev{made_up(f.id, s, 8u), made_up(f.id, s, 9u), made_up(f.id, s, 10u)};
    }
    slgplan::NestedFilterPlan np;
    slgplan::plan_nested_filter_trees(views, reject.data(), filter_live, n_filters, pviews, nviews, n_segs, trees, n_trees, np);
    static_assert(sizeof(slg::NestedScopeDev) == 16 && sizeof(slg::FilterNodeDev) == 32, "the words the caller reads");
    if (scope_rows && np.scopes.size() <= scopes_cap)
      std::memcpy(scope_rows, np.scopes.data(), np.scopes.size() * sizeof(slg::NestedScopeDev));
    if (nodes && np.nodes.size() <= nodes_cap) std::memcpy(nodes, np.nodes.data(), np.nodes.size() * sizeof(slg::FilterNodeDev));
    if (levels && np.level_begin.size() <= levels_cap) std::memcpy(levels, np.level_begin.data(), np.level_begin.size() * 4);
    if (words && np.words.size() <= words_cap && !np.words.empty()) std::memcpy(words, np.words.data(), np.words.size() * 4);
    if (counts) {
      counts[0] = (uint32_t)np.scopes.size();
      counts[1] = (uint32_t)np.nodes.size();
      counts[2] = (uint32_t)np.level_begin.size();
      counts[3] = (uint32_t)np.words.size();
      counts[4] = n_segs ? (uint32_t)(np.paths.size() / n_segs) : 0u;
      counts[5] = n_segs ? (uint32_t)(np.ncols.size() / n_segs) : 0u;
    }
    return SLG_OK;
  } catch (const slgplan::SlgError &e) {
    if (err && err_len) {
      std::strncpy(err, e.what(), err_len - 1);
      err[err_len - 1] = 0;
    }
    return e.code;
  }
}

// the bucket function of a date_histogram node (slg::date_bucket_id, slg_date.hpp: what the planner's row range and
// the aggregation kernels run) over n values: ids[i] = the bucket id of vals[i] under unit (SLG_DATE_*), step and
// offset (i64 ms; step is read for SLG_DATE_FIXED only); ymd[3 i ..] = year, month, day of the UTC day that holds
// vals[i] - offset (slg::date_civil).  Either output may be NULL.  0, or SLG_ERR_INVALID (an unknown unit, a fixed
// step < 1, vals NULL with n > 0)
int slgp_date_buckets(uint32_t unit, int64_t step, int64_t offset, const int64_t *vals, uint64_t n, int64_t *ids,
                      int32_t *ymd) {
  if (unit > slg::kDateYear || (unit == slg::kDateFixed && step < 1) || (n && !vals)) return SLG_ERR_INVALID;
  for (uint64_t i = 0; i < n; i++) {
    if (ids) ids[i] = slg::date_bucket_id(unit, step, offset, vals[i]);
    if (ymd) {
      long long y;
      uint32_t m, d;
      slg::date_civil(slg::date_floor_div(vals[i] - offset, slg::kDateDayMs), y, m, d);
      ymd[3 * i] = (int32_t)y;
      ymd[3 * i + 1] = (int32_t)m;
      ymd[3 * i + 2] = (int32_t)d;
    }
  }
  return SLG_OK;
}

// the host checks of slg_index_set_positions over a segment of n_postings postings.  0, or a negative error code
int slgp_check_positions(uint64_t n_postings, const uint64_t *pos_offsets, const uint32_t *positions, char *err,
                         uint32_t err_len) {
  try {
    slgplan::check_positions(n_postings, pos_offsets, positions);
    return SLG_OK;
  } catch (const slgplan::SlgError &e) {
    if (err && err_len) {
      std::strncpy(err, e.what(), err_len - 1);
      err[err_len - 1] = 0;
    }
    return e.code;
  }
}

}  // extern "C"
