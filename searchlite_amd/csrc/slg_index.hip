// slg_index.hip — the index: creation and destruction, tuning, segment staging, the immutable states and
// their updates (filters, filter trees, sort fields, vector fields, tombstones, segments), profiling switches.
//
// The host units (this one, slg_batch.hip, slg_shard.hip, slg_rerank.hip, slg_vsearch.hip; what they
// share: slg_host.hpp) are the host side of the C ABI declared in include/searchlite_gpu.h.  They
// mirror, for the GPU-eligible request shape, what IndexReader::search_segment does before and after
// the scorer call (searchlite-core/src/api/reader.rs:2971-3000 build the ScoredTerm list; :3075-3099
// call the scorer; :2776-2778 merge across segments), but for a whole batch of queries at once.  The
// product path has NO CPU fallback: every entry point either runs the HIP kernels or fails with an
// error code.
#include "slg_host.hpp"

#include <cmath>
#include <cstdlib>

#include "slg_filter.hpp"
#include "slg_nested.hpp"
#include "slg_stage.hpp"

slghost::LastError &slghost::last_error() {
  thread_local LastError le;
  return le;
}
using namespace slghost;

namespace {

// (the environment is read in slg_tuning_default() only)
uint32_t env_u32(const char *name, uint32_t dflt) {
  const char *v = std::getenv(name);
  if (!v || !*v) return dflt;
  return (uint32_t)std::strtoul(v, nullptr, 10);
}
int32_t env_i32(const char *name, int32_t dflt) {
  const char *v = std::getenv(name);
  if (!v || !*v) return dflt;
  return (int32_t)std::strtol(v, nullptr, 10);
}

void validate_segment(const slg_segment_desc &d, uint32_t si, bool deep) {
  const std::string pfx = "segment " + std::to_string(si) + ": ";
  SLG_REQUIRE(d.term_offsets != nullptr, pfx + "term_offsets is NULL");
  SLG_REQUIRE(d.n_fields >= 1 && d.field_avgdl && d.field_doc_len, pfx + "field arrays missing");
  SLG_REQUIRE(d.term_offsets[0] == 0, pfx + "term_offsets[0] != 0");
  const uint64_t P = d.term_offsets[d.n_terms];
  SLG_REQUIRE(P == 0 || (d.doc_ids && d.tfs), pfx + "doc_ids/tfs missing");
  for (uint32_t t = 0; t < d.n_terms; t++) {
    const uint64_t a = d.term_offsets[t], b = d.term_offsets[t + 1];
    SLG_REQUIRE(b >= a, pfx + "term_offsets not monotone");
    SLG_REQUIRE(b - a <= 0xFFFFFFFEull, pfx + "posting list too long");
    if (d.term_field) SLG_REQUIRE(d.term_field[t] < d.n_fields, pfx + "term_field out of range");
    // The kernels index per-doc bitmaps with the raw doc id and the planner interpolates on
    // doc / n_docs, so ids must be < n_docs: checked on every posting, or (validate == 0, where
    // the caller vouches for increasing ids) on the last = largest posting of each list.
    if (deep) {
      for (uint64_t i = a; i < b; i++) {
        SLG_REQUIRE(d.doc_ids[i] < d.n_docs,
                    pfx + "doc id >= n_docs in term " + std::to_string(t));
        SLG_REQUIRE(i == a || d.doc_ids[i] > d.doc_ids[i - 1],
                    pfx + "doc ids not strictly increasing in term " + std::to_string(t));
      }
    } else if (b > a) {
      SLG_REQUIRE(d.doc_ids[b - 1] < d.n_docs, pfx + "doc id >= n_docs in term " + std::to_string(t));
    }
  }
  if (d.vec_dim) {
    SLG_REQUIRE(d.vec_offsets && (d.vec_values || d.vec_rows == 0), pfx + "vector arrays missing");
    SLG_REQUIRE(d.vec_metric == SLG_METRIC_COSINE || d.vec_metric == SLG_METRIC_L2,
                pfx + "bad vec_metric");
    if (deep)
      for (uint32_t i = 0; i < d.n_docs; i++)
        SLG_REQUIRE(d.vec_offsets[i] == SLG_NO_VECTOR || d.vec_offsets[i] < d.vec_rows,
                    pfx + "vec_offsets out of range");
  }
}

// The version of a staged segment for (deleted bitmap, live_docs): impacts (stage_impacts_kernel:
// query/bm25.rs:1-6 with idf from the host's logf), champion bounds, host mirror.  At creation the
// kernel also scatters the uploaded doc ids into the padded layout (docs_in != nullptr); for an
// update it reads them back from there.  Temporaries of a non-updatable store are passed in `tmp`.
struct StageTemps {
  const uint32_t *docs_in = nullptr;   // [P] unpadded doc ids as uploaded (creation only)
};
void derive_version(slg_index *ix, const std::shared_ptr<PostingStore> &ps, SegHost &sh, const uint8_t *deleted,
                    float docs, const StageTemps &tmp) {
  hipStream_t st = ix->stream;
  sh.store = ps;
  sh.n_docs = ps->n_docs;
  sh.n_terms = ps->n_terms;
  sh.n_postings = ps->n_postings;
  sh.null_idx = ps->null_idx;
  sh.docs = docs;
  const uint64_t P = ps->n_postings;
  const uint64_t P_pad = P + (uint64_t)slg::kListPad * (uint64_t)ps->n_terms + (uint64_t)slg::kNullRun;
  sh.d_imps.alloc(P_pad * 4, &ix->pool);
  SLG_HIP(hipMemsetAsync(sh.d_imps.p, 0, P_pad * 4, st));
  if (deleted) {
    const size_t words = ((size_t)ps->n_docs + 31) / 32;
    std::vector<uint32_t> w(words ? words : 1, 0u);
    std::memcpy(w.data(), deleted, ((size_t)ps->n_docs + 7) / 8);
    sh.d_deleted.alloc(w.size() * 4, &ix->pool);
    SLG_HIP(hipMemcpy(sh.d_deleted.p, w.data(), w.size() * 4, hipMemcpyHostToDevice));
  }
  if (P == 0) return;
  // idf per term: query/bm25.rs:2 with df = postings.len() as f32 (wand.rs:108,471)
  std::vector<float> idf(ps->n_terms);
  for (uint32_t t = 0; t < ps->n_terms; t++) {
    const float df = (float)(uint32_t)(ps->term_offsets[t + 1] - ps->term_offsets[t]);
    idf[t] = fmaxf(logf((docs - df + 0.5f) / (df + 0.5f)), 0.0f) + 1.0f;
  }
  DevBuf d_idf;
  d_idf.alloc((size_t)ps->n_terms * 4, &ix->pool);
  SLG_HIP(hipMemcpyAsync(d_idf.p, idf.data(), (size_t)ps->n_terms * 4, hipMemcpyHostToDevice, st));
  slg::StageParams sp{};
  sp.n_postings = P;
  sp.n_terms = ps->n_terms;
  sp.n_docs = ps->n_docs;
  sp.term_offsets = ps->d_offs.as<uint64_t>();
  sp.docs = tmp.docs_in;
  sp.docs_out = ps->d_docs.as<uint32_t>();
  sp.tfs = ps->d_tfs.as<uint32_t>();
  sp.term_idf = d_idf.as<float>();
  sp.term_field = ps->has_term_field ? ps->d_tfield.as<uint16_t>() : nullptr;
  sp.field_doc_len = ps->d_lenptrs.as<const float *>();
  sp.field_avgdl = ps->d_avgdl.as<float>();
  sp.k1 = ps->k1;
  sp.b = ps->b;
  sp.imps = sh.d_imps.as<float>();
  const uint64_t want = (P + 255) / 256;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(want, 256ull * 32);
  hipLaunchKernelGGL(slg::stage_impacts_kernel, dim3(blocks), dim3(256), 0, st, sp);
  SLG_HIP(hipGetLastError());
  if (ix->tune.champions) {
    sh.d_champ.alloc((size_t)ps->n_terms * slg::kChampions * 4, &ix->pool);
    slg::ChampParams cp{};
    cp.term_offsets = ps->d_offs.as<uint64_t>();
    cp.imps = sh.d_imps.as<float>();
    cp.docs = ps->d_docs.as<uint32_t>();
    cp.deleted = sh.d_deleted.as<uint32_t>();
    cp.champ = sh.d_champ.as<float>();
    cp.n_terms = ps->n_terms;
    const uint32_t cblocks = std::min<uint32_t>((ps->n_terms + 3) / 4, 256u * 16);
    hipLaunchKernelGGL(slg::stage_champions_kernel, dim3(cblocks ? cblocks : 1), dim3(256), 0, st, cp);
    SLG_HIP(hipGetLastError());
  }
  SLG_HIP(hipStreamSynchronize(st));  // d_idf dies here
  if (sh.d_champ.p) {
    sh.champ.resize((size_t)ps->n_terms * slg::kChampions);
    SLG_HIP(hipMemcpy(sh.champ.data(), sh.d_champ.p, sh.champ.size() * 4, hipMemcpyDeviceToHost));
  }
}

std::shared_ptr<SegHost> stage_segment(slg_index *ix, const slg_segment_desc &d) {
  hipStream_t st = ix->stream;
  auto ps = std::make_shared<PostingStore>();
  ps->n_docs = d.n_docs;
  ps->n_terms = d.n_terms;
  ps->n_fields = d.n_fields;
  ps->term_offsets.assign(d.term_offsets, d.term_offsets + d.n_terms + 1);
  ps->avgdl.assign(d.field_avgdl, d.field_avgdl + d.n_fields);
  ps->k1 = d.k1;
  ps->b = d.b;
  ps->has_term_field = d.term_field != nullptr;
  ps->updatable = ix->tune.updatable != 0;
  const uint64_t P = ps->term_offsets[d.n_terms];
  ps->n_postings = P;

  // padded layout (SegDev): every list is followed by kListPad sentinel entries, + a run of kNullRun
  // at the end (null_idx): the scoring kernels load whole 64-lane slots starting at any posting
  const uint64_t P_pad = P + (uint64_t)slg::kListPad * (uint64_t)d.n_terms + (uint64_t)slg::kNullRun;
  ps->null_idx = P + (uint64_t)slg::kListPad * d.n_terms;
  ps->d_docs.alloc(P_pad * 4, &ix->pool);
  SLG_HIP(hipMemsetAsync(ps->d_docs.p, 0xFF, P_pad * 4, st));
  DevBuf d_docs_in;  // the uploaded (unpadded) doc ids: staging only
  if (P > 0) {
    d_docs_in.alloc(P * 4, &ix->pool);
    ps->d_tfs.alloc(P * 4, &ix->pool);
    SLG_HIP(hipMemcpyAsync(d_docs_in.p, d.doc_ids, P * 4, hipMemcpyHostToDevice, st));
    SLG_HIP(hipMemcpyAsync(ps->d_tfs.p, d.tfs, P * 4, hipMemcpyHostToDevice, st));
    ps->d_offs.alloc(((size_t)d.n_terms + 1) * 8, &ix->pool);
    SLG_HIP(hipMemcpyAsync(ps->d_offs.p, ps->term_offsets.data(), ((size_t)d.n_terms + 1) * 8,
                           hipMemcpyHostToDevice, st));
    if (d.term_field) {
      ps->d_tfield.alloc((size_t)d.n_terms * 2, &ix->pool);
      SLG_HIP(hipMemcpyAsync(ps->d_tfield.p, d.term_field, (size_t)d.n_terms * 2, hipMemcpyHostToDevice, st));
    }
    ps->d_avgdl.alloc((size_t)d.n_fields * 4, &ix->pool);
    SLG_HIP(hipMemcpyAsync(ps->d_avgdl.p, d.field_avgdl, (size_t)d.n_fields * 4, hipMemcpyHostToDevice, st));
    ps->d_lens.resize(d.n_fields);
    std::vector<const float *> lenptrs(d.n_fields, nullptr);
    for (uint32_t f = 0; f < d.n_fields; f++) {
      if (d.field_doc_len[f] && d.n_docs) {
        ps->d_lens[f].alloc((size_t)d.n_docs * 4, &ix->pool);
        SLG_HIP(hipMemcpyAsync(ps->d_lens[f].p, d.field_doc_len[f], (size_t)d.n_docs * 4, hipMemcpyHostToDevice, st));
        lenptrs[f] = ps->d_lens[f].as<float>();
      }
    }
    ps->d_lenptrs.alloc((size_t)d.n_fields * sizeof(float *), &ix->pool);
    SLG_HIP(hipMemcpy(ps->d_lenptrs.p, lenptrs.data(), (size_t)d.n_fields * sizeof(float *), hipMemcpyHostToDevice));
  }
  auto sh = std::make_shared<SegHost>();
  StageTemps tmp;
  tmp.docs_in = d_docs_in.as<uint32_t>();
  derive_version(ix, ps, *sh, d.deleted, d.docs, tmp);  // (synchronises the stream when P > 0)
  if (!ps->updatable) {  // what only an update would read again
    ps->d_tfs.release();
    ps->d_offs.release();
    ps->d_tfield.release();
    ps->d_avgdl.release();
    ps->d_lenptrs.release();
    ps->d_lens.clear();
  }
  if (d.vec_dim) {
    ps->vec_dim = d.vec_dim;
    ps->vec_rows = d.vec_rows;
    ps->vec_metric = d.vec_metric;
    ps->d_vec_offsets.alloc((size_t)d.n_docs * 4, &ix->pool);
    if (d.n_docs)
      SLG_HIP(hipMemcpy(ps->d_vec_offsets.p, d.vec_offsets, (size_t)d.n_docs * 4, hipMemcpyHostToDevice));
    const size_t vb = (size_t)d.vec_rows * d.vec_dim * 4;
    ps->d_vec_values.alloc(vb, &ix->pool);
    if (vb) SLG_HIP(hipMemcpy(ps->d_vec_values.p, d.vec_values, vb, hipMemcpyHostToDevice));
  }
  SLG_HIP(hipStreamSynchronize(st));
  return sh;
}

// the device tables of a state (segment descriptors, vector stores, reject-bitmap pointers): small,
// rebuilt for every state
void finish_state(slg_index *ix, IndexState &s) {
  const size_t n_segs = s.segs.size();
  s.device = ix->device;
  std::vector<slg::SegDev> sd(n_segs);
  std::vector<slg::VecSegDev> vd(n_segs);
  // a segment without vectors takes the field's metric (the last one's, as field_facts reports it): its
  // docs score missing_vector_score of the field's metric, not of the descriptor's unchecked vec_metric
  int32_t field_metric = 0;
  for (size_t i = 0; i < n_segs; i++)
    if (s.segs[i]->store->vec_dim) field_metric = s.segs[i]->store->vec_metric;
  for (size_t i = 0; i < n_segs; i++) {
    const SegHost &sh = *s.segs[i];
    sd[i].docs = sh.store->d_docs.as<uint32_t>();
    sd[i].imps = sh.d_imps.as<float>();
    sd[i].deleted = sh.d_deleted.as<uint32_t>();
    sd[i].champ = sh.d_champ.as<float>();
    sd[i].n_docs = sh.n_docs;
    sd[i].pad = 0;
    sd[i].null_idx = sh.null_idx;
    vd[i].offsets = sh.store->d_vec_offsets.as<uint32_t>();
    vd[i].values = sh.store->d_vec_values.as<float>();
    vd[i].n_docs = sh.n_docs;
    vd[i].dim = sh.store->vec_dim;
    vd[i].metric = sh.store->vec_dim ? sh.store->vec_metric : field_metric;
    vd[i].pad = 0;
  }
  s.d_segs.alloc(std::max<size_t>(n_segs, 1) * sizeof(slg::SegDev), &ix->pool);
  s.d_vsegs.alloc(std::max<size_t>(n_segs, 1) * sizeof(slg::VecSegDev), &ix->pool);
  if (n_segs) {
    SLG_HIP(hipMemcpy(s.d_segs.p, sd.data(), n_segs * sizeof(slg::SegDev), hipMemcpyHostToDevice));
    SLG_HIP(hipMemcpy(s.d_vsegs.p, vd.data(), n_segs * sizeof(slg::VecSegDev), hipMemcpyHostToDevice));
  }
  for (auto &vfp : s.vfields) {  // (the field objects of a new state are fresh copies: see copy_state)
    VecFieldHost &vf = *vfp;
    std::vector<slg::VecSegDev> fv(n_segs);
    for (size_t i = 0; i < n_segs; i++) {
      fv[i] = slg::VecSegDev{nullptr, nullptr, s.segs[i]->n_docs, 0u, vf.metric, 0u};
      if (i < vf.per_seg.size() && vf.per_seg[i]) {
        fv[i].offsets = vf.per_seg[i]->offsets.as<uint32_t>();
        fv[i].values = vf.per_seg[i]->values.as<float>();
        fv[i].dim = vf.per_seg[i]->dim;
      }
    }
    vf.d_vsegs.alloc(std::max<size_t>(n_segs, 1) * sizeof(slg::VecSegDev), &ix->pool);
    if (n_segs) SLG_HIP(hipMemcpy(vf.d_vsegs.p, fv.data(), n_segs * sizeof(slg::VecSegDev), hipMemcpyHostToDevice));
  }
  for (auto &vcp : s.vcopies) {  // (fresh copies too)
    VecCopyField &vc = *vcp.second;
    vc.per_seg.resize(n_segs);
    std::vector<slg::VecCopyDev> cv(n_segs, slg::VecCopyDev{nullptr, nullptr, 0u, 0u});
    for (size_t i = 0; i < n_segs; i++)
      if (vc.per_seg[i])
        cv[i] = slg::VecCopyDev{vc.per_seg[i]->rows.as<uint16_t>(), vc.per_seg[i]->norms.as<float>(),
                                vc.per_seg[i]->dim_pad, 0u};
    vc.d_csegs.alloc(std::max<size_t>(n_segs, 1) * sizeof(slg::VecCopyDev), &ix->pool);
    if (n_segs) SLG_HIP(hipMemcpy(vc.d_csegs.p, cv.data(), n_segs * sizeof(slg::VecCopyDev), hipMemcpyHostToDevice));
  }
  for (auto &vlp : s.vlists) {  // (fresh copies too) the inverted-file lists' tables
    VecListField &vl = *vlp.second;
    const uint32_t f = vlp.first;
    vl.per_seg.resize(n_segs);
    std::vector<slg::VecListDev> lv(n_segs, slg::VecListDev{nullptr, nullptr, 0u, 0u});
    std::vector<slg::VecSegDev> cv(n_segs);
    std::vector<slg::SegDev> pv(n_segs, slg::SegDev{});
    std::vector<uint32_t> lbase(n_segs + 1, 0u);
    std::vector<slg::IvfUncl> uv;
    const int32_t metric = f == 0 ? field_metric : (f <= s.vfields.size() ? s.vfields[f - 1]->metric : 0);
    vl.total_lists = vl.max_len = vl.uncl_slots = 0;
    for (size_t i = 0; i < n_segs; i++) {
      lbase[i] = vl.total_lists;
      cv[i] = slg::VecSegDev{nullptr, nullptr, 0u, 0u, metric, 0u};
      const bool has_vectors = f == 0 ? s.segs[i]->store->vec_dim != 0
                                      : (f <= s.vfields.size() && i < s.vfields[f - 1]->per_seg.size() &&
                                         s.vfields[f - 1]->per_seg[i]);
      if (vl.per_seg[i] && vl.per_seg[i]->n_lists) {
        const VecListSeg &ls = *vl.per_seg[i];
        lv[i] = slg::VecListDev{ls.list_begin.as<uint32_t>(), ls.docs.as<uint32_t>(), ls.n_lists, 0u};
        cv[i] = slg::VecSegDev{ls.iota.as<uint32_t>(), ls.centroids.as<float>(), ls.n_lists, ls.dim, metric, 0u};
        pv[i].n_docs = ls.n_lists;
        vl.total_lists += ls.n_lists;
        vl.max_len = std::max(vl.max_len, ls.max_len);
      } else if (has_vectors && s.segs[i]->n_docs) {
        // chunks of whole scan tiles (128 docs), at most kIvfUnclChunks of them
        const uint32_t nd = s.segs[i]->n_docs, tiles = (nd + 127u) / 128u;
        const uint32_t want = std::min<uint32_t>(tiles, slg::kIvfUnclChunks), chunk = ((tiles + want - 1) / want) * 128u;
        uv.push_back(slg::IvfUncl{(uint32_t)i, nd, chunk, vl.uncl_slots});
        vl.uncl_slots += (nd + chunk - 1) / chunk;
      }
    }
    lbase[n_segs] = vl.total_lists;
    vl.n_uncl = (uint32_t)uv.size();
    vl.d_lsegs.alloc(std::max<size_t>(n_segs, 1) * sizeof(slg::VecListDev), &ix->pool);
    vl.d_csegs.alloc(std::max<size_t>(n_segs, 1) * sizeof(slg::VecSegDev), &ix->pool);
    vl.d_psegs.alloc(std::max<size_t>(n_segs, 1) * sizeof(slg::SegDev), &ix->pool);
    vl.d_list_base.alloc(lbase.size() * 4, &ix->pool);
    vl.d_uncl.alloc(std::max<size_t>(uv.size(), 1) * sizeof(slg::IvfUncl), &ix->pool);
    if (n_segs) {
      SLG_HIP(hipMemcpy(vl.d_lsegs.p, lv.data(), n_segs * sizeof(slg::VecListDev), hipMemcpyHostToDevice));
      SLG_HIP(hipMemcpy(vl.d_csegs.p, cv.data(), n_segs * sizeof(slg::VecSegDev), hipMemcpyHostToDevice));
      SLG_HIP(hipMemcpy(vl.d_psegs.p, pv.data(), n_segs * sizeof(slg::SegDev), hipMemcpyHostToDevice));
    }
    SLG_HIP(hipMemcpy(vl.d_list_base.p, lbase.data(), lbase.size() * 4, hipMemcpyHostToDevice));
    if (!uv.empty()) SLG_HIP(hipMemcpy(vl.d_uncl.p, uv.data(), uv.size() * sizeof(slg::IvfUncl), hipMemcpyHostToDevice));
  }
  s.positions.resize(n_segs);  // (a new state of a new segment list: no positions where none were set)
  std::vector<slg::PosSegDev> pd(n_segs);
  for (size_t i = 0; i < n_segs; i++)
    if (s.positions[i]) pd[i] = slg::PosSegDev{s.positions[i]->offs.as<uint32_t>(), s.positions[i]->pos.as<uint32_t>()};
  s.d_pos_segs.alloc(std::max<size_t>(n_segs, 1) * sizeof(slg::PosSegDev), &ix->pool);
  if (n_segs) SLG_HIP(hipMemcpy(s.d_pos_segs.p, pd.data(), n_segs * sizeof(slg::PosSegDev), hipMemcpyHostToDevice));
  s.terms.resize(n_segs);  // (the same for the dictionaries)
  std::vector<slg::ExpandSegDev> td(n_segs, slg::ExpandSegDev{nullptr, nullptr, nullptr});
  for (size_t i = 0; i < n_segs; i++)
    if (s.terms[i]) td[i] = slg::ExpandSegDev{s.terms[i]->bytes.as<unsigned char>(), s.terms[i]->offs.as<uint32_t>(), s.terms[i]->nchars.as<uint8_t>()};
  s.d_term_segs.alloc(std::max<size_t>(n_segs, 1) * sizeof(slg::ExpandSegDev), &ix->pool);
  if (n_segs) SLG_HIP(hipMemcpy(s.d_term_segs.p, td.data(), n_segs * sizeof(slg::ExpandSegDev), hipMemcpyHostToDevice));
  std::vector<slg::SuggestSegDev> ud(n_segs, slg::SuggestSegDev{nullptr, nullptr, nullptr, nullptr});
  for (size_t i = 0; i < n_segs; i++)
    if (s.terms[i]) ud[i] = slg::SuggestSegDev{td[i].bytes, td[i].offs, td[i].nchars, s.terms[i]->d_df.as<uint32_t>()};
  s.d_suggest_segs.alloc(std::max<size_t>(n_segs, 1) * sizeof(slg::SuggestSegDev), &ix->pool);
  if (n_segs) SLG_HIP(hipMemcpy(s.d_suggest_segs.p, ud.data(), n_segs * sizeof(slg::SuggestSegDev), hipMemcpyHostToDevice));
  for (auto &tfp : s.text_fields) {  // (the field objects of a new state are fresh copies: see copy_state)
    TextFieldHost &tf = *tfp.second;
    tf.per_seg.resize(n_segs);
    std::vector<slg::TextSegDev> tv(n_segs, slg::TextSegDev{nullptr, nullptr, nullptr, 0u, 0u});
    for (size_t i = 0; i < n_segs; i++)
      if (tf.per_seg[i])
        tv[i] = slg::TextSegDev{tf.per_seg[i]->bytes.as<uint8_t>(), tf.per_seg[i]->offs.as<uint64_t>(),
                                tf.per_seg[i]->non_ascii.as<uint32_t>(), tf.per_seg[i]->n_docs, 0u};
    tf.d_tsegs.alloc(std::max<size_t>(n_segs, 1) * sizeof(slg::TextSegDev), &ix->pool);
    if (n_segs) SLG_HIP(hipMemcpy(tf.d_tsegs.p, tv.data(), n_segs * sizeof(slg::TextSegDev), hipMemcpyHostToDevice));
  }
  std::vector<uint32_t> base(n_segs + 1, 0u);
  uint64_t acc = 0;
  for (size_t i = 0; i < n_segs; i++) {
    base[i] = (uint32_t)std::min<uint64_t>(acc, 0xFFFFFFFFull);
    acc += s.segs[i]->n_docs;
  }
  base[n_segs] = (uint32_t)std::min<uint64_t>(acc, 0xFFFFFFFFull);
  s.total_docs = acc;
  s.d_doc_base.alloc(base.size() * 4, &ix->pool);
  SLG_HIP(hipMemcpy(s.d_doc_base.p, base.data(), base.size() * 4, hipMemcpyHostToDevice));
  s.reject_host.assign(s.filters.size() * n_segs, nullptr);
  for (size_t f = 0; f < s.filters.size(); f++)
    if (s.filters[f])
      for (size_t i = 0; i < n_segs && i < s.filters[f]->per_seg.size(); i++)
        if (s.filters[f]->per_seg[i]) s.reject_host[f * n_segs + i] = s.filters[f]->per_seg[i]->as<uint32_t>();
  s.d_reject_table.alloc(std::max<size_t>(s.reject_host.size(), 1) * sizeof(void *), &ix->pool);
  if (!s.reject_host.empty())
    SLG_HIP(hipMemcpy(s.d_reject_table.p, s.reject_host.data(), s.reject_host.size() * sizeof(void *),
                      hipMemcpyHostToDevice));
}

// the next state: the current one's segments / fields / filters (shared), the device tables not yet built
std::unique_ptr<IndexState> copy_state(const IndexState &cur) {
  auto n = std::make_unique<IndexState>();
  n->generation = cur.generation + 1;
  n->device = cur.device;
  n->segs = cur.segs;
  n->filters = cur.filters;
  n->sort_fields = cur.sort_fields;
  n->agg_fields = cur.agg_fields;
  n->nested_paths = cur.nested_paths;
  n->nested_fields = cur.nested_fields;
  n->positions = cur.positions;
  n->terms = cur.terms;
  for (auto &vf : cur.vfields) {  // the per-state table d_vsegs is rebuilt: own object, shared stores
    auto c = std::make_shared<VecFieldHost>();
    c->dim = vf->dim;
    c->metric = vf->metric;
    c->per_seg = vf->per_seg;
    n->vfields.push_back(std::move(c));
  }
  for (auto &vc : cur.vcopies) {  // the same for the bf16 copies' d_csegs
    auto c = std::make_shared<VecCopyField>();
    c->per_seg = vc.second->per_seg;
    n->vcopies.emplace(vc.first, std::move(c));
  }
  for (auto &vl : cur.vlists) {  // the same for the inverted-file lists' tables
    auto c = std::make_shared<VecListField>();
    c->per_seg = vl.second->per_seg;
    n->vlists.emplace(vl.first, std::move(c));
  }
  for (auto &tf : cur.text_fields) {  // the same for the text fields' d_tsegs
    auto c = std::make_shared<TextFieldHost>();
    c->per_seg = tf.second->per_seg;
    n->text_fields.emplace(tf.first, std::move(c));
  }
  return n;
}

void publish(slg_index *ix, std::unique_ptr<IndexState> ns) {
  std::shared_ptr<const IndexState> keep;  // (the old state may die here: outside the lock)
  std::shared_ptr<const IndexState> fresh(std::move(ns));
  {
    std::lock_guard<std::mutex> lk(ix->mu);
    keep.swap(ix->state);
    ix->state = fresh;
    ix->generation.store(fresh->generation, std::memory_order_release);
  }
}

// One change of the index's state: updates are serialised by update_mu; change(cur, next) turns a copy
// of the current state into the next one on the index's device (whatever it throws leaves the index as it
// was), then the device tables are built and the state is published.  Batches prepared on earlier states
// keep theirs: nobody waits for the device here.  new_generation false: a change no manifest snapshot
// sees (filters, sort fields, vector fields).
template <typename F>
void update_state(slg_index *ix, bool new_generation, F &&change) {
  std::lock_guard<std::mutex> ulk(ix->update_mu);
  const auto cur = ix->snapshot();
  DeviceGuard g(ix->device);
  auto ns = copy_state(*cur);
  if (!new_generation) ns->generation = cur->generation;
  change(*cur, *ns);
  finish_state(ix, *ns);
  publish(ix, std::move(ns));
}

// every per-segment table of a state (filters, sort fields, vector fields) reshaped by op when the
// segment list changes; filters and sort fields are shared with earlier states: copy on write
template <typename Op>
void reshape_per_segment(IndexState &ns, Op op) {
  for (auto &f : ns.filters)
    if (f) {
      auto nf = std::make_shared<FilterData>(*f);
      op(nf->per_seg);
      f = std::move(nf);
    }
  for (auto &sf : ns.sort_fields) {
    auto nf = std::make_shared<SortFieldData>(*sf.second);
    op(nf->per_seg);
    sf.second = std::move(nf);
  }
  for (auto &af : ns.agg_fields) {
    auto nf = std::make_shared<AggFieldData>(*af.second);
    op(nf->per_seg);
    op(nf->ranks);
    nf->refold();  // (a histogram's dense id range follows the minimum and maximum of the segments left)
    af.second = std::move(nf);
  }
  for (auto &np : ns.nested_paths) {
    auto nf = std::make_shared<NestedPathData>(*np.second);
    op(nf->per_seg);
    np.second = std::move(nf);
  }
  for (auto &nc : ns.nested_fields) {
    auto nf = std::make_shared<NestedFieldData>(*nc.second);
    op(nf->per_seg);
    nc.second = std::move(nf);
  }
  for (auto &vf : ns.vfields) op(vf->per_seg);  // (the field objects of a new state are fresh copies)
  for (auto &vc : ns.vcopies) op(vc.second->per_seg);  // (fresh copies too)
  for (auto &vl : ns.vlists) op(vl.second->per_seg);  // (fresh copies too)
  op(ns.positions);  // (the state's own vector; the stores are shared)
  op(ns.terms);
  for (auto &tf : ns.text_fields) op(tf.second->per_seg);  // (fresh copies too)
}

size_t state_device_bytes(const IndexState &s) {
  size_t n = s.d_segs.bytes + s.d_vsegs.bytes + s.d_reject_table.bytes + s.d_doc_base.bytes + s.d_pos_segs.bytes;
  for (auto &ps : s.positions)
    if (ps) n += ps->offs.bytes + ps->pos.bytes;
  n += s.d_term_segs.bytes + s.d_suggest_segs.bytes;
  for (auto &ts : s.terms)
    if (ts) n += ts->device_bytes();
  for (auto &tf : s.text_fields) {
    n += tf.second->d_tsegs.bytes;
    for (auto &t : tf.second->per_seg)
      if (t) n += t->device_bytes();
  }
  for (auto &sh : s.segs) n += sh->device_bytes() + sh->store->device_bytes();
  for (auto &f : s.filters)
    if (f)
      for (auto &b : f->per_seg)
        if (b) n += b->bytes;
  for (auto &sf : s.sort_fields)
    for (auto &c : sf.second->per_seg)
      if (c) n += c->key[0].bytes + c->key[1].bytes + c->present.bytes;
  for (auto &af : s.agg_fields) {
    for (auto &c : af.second->per_seg)
      if (c) n += c->offs.bytes + c->vals.bytes;
    for (auto &r : af.second->ranks)
      if (r) n += r->bytes;
    if (af.second->dict) n += af.second->dict->vals.bytes;
  }
  for (auto &np : s.nested_paths)
    for (auto &c : np.second->per_seg)
      if (c) n += c->device_bytes();
  for (auto &nc : s.nested_fields)
    for (auto &c : nc.second->per_seg)
      if (c) n += c->device_bytes();
  for (auto &vf : s.vfields) {
    n += vf->d_vsegs.bytes;
    for (auto &v : vf->per_seg)
      if (v) n += v->offsets.bytes + v->values.bytes;
  }
  for (auto &vc : s.vcopies) {
    n += vc.second->d_csegs.bytes;
    for (auto &c : vc.second->per_seg)
      if (c) n += c->rows.bytes + c->norms.bytes;
  }
  for (auto &vl : s.vlists) {
    const VecListField &f = *vl.second;
    n += f.d_lsegs.bytes + f.d_csegs.bytes + f.d_psegs.bytes + f.d_list_base.bytes + f.d_uncl.bytes;
    for (auto &l : f.per_seg)
      if (l) n += l->list_begin.bytes + l->docs.bytes + l->centroids.bytes + l->iota.bytes;
  }
  return n;
}

}  // namespace

namespace {
// the store of segment s in vector field `field` of a state (*dim 0: the segment has no vectors in the field)
void vec_store_of(const IndexState &cur, uint32_t field, size_t s, const uint32_t **offs, const float **vals,
                  uint32_t *rows, uint32_t *dim, int32_t *metric) {
  *dim = 0;
  if (field == 0) {
    const PostingStore &ps = *cur.segs[s]->store;
    if (!ps.vec_dim) return;
    *offs = ps.d_vec_offsets.as<uint32_t>();
    *vals = ps.d_vec_values.as<float>();
    *rows = ps.vec_rows;
    *dim = ps.vec_dim;
    *metric = ps.vec_metric;
  } else {
    const VecFieldHost &vf = *cur.vfields[field - 1];
    if (s >= vf.per_seg.size() || !vf.per_seg[s]) return;
    const VecSegStore &st = *vf.per_seg[s];
    *offs = st.offsets.as<uint32_t>();
    *vals = st.values.as<float>();
    *rows = st.n_rows;
    *dim = st.dim;
    *metric = vf.metric;
  }
}
}  // namespace

extern "C" {

uint32_t slg_abi_version(void) { return SLG_ABI_VERSION; }

const char *slg_last_error(void) { return last_error().msg.c_str(); }
int slg_last_error_code(void) { return last_error().code; }

int slg_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    last_error().msg = std::string("hipGetDeviceCount: ") + hipGetErrorString(e);
    return SLG_ERR_DEVICE;
  }
  return n;
}

void slg_tuning_default(slg_tuning *t) {
  if (!t) return;
  std::memset(t, 0, sizeof(*t));
  t->struct_size = (uint32_t)sizeof(slg_tuning);
  t->validate = env_i32("SLG_VALIDATE", 1) != 0;
  t->champions = env_i32("SLG_NO_CHAMPIONS", 0) == 0;
  t->allow_any_arch = env_i32("SLG_ALLOW_ANY_ARCH", 0) != 0;
  t->pruning = env_i32("SLG_MAXSCORE", -1);
  t->uniform_max_terms = env_u32("SLG_UNIFORM_MAX_TERMS", 8);
  t->uniform_round_target = env_u32("SLG_UNIFORM_ROUND_TARGET", 0);
  t->multi_round_target = env_u32("SLG_MULTI_ROUND_TARGET", slg::kMultiTarget);
  t->probe_target = env_u32("SLG_PROBE_TARGET", 2048);
  t->rounds_per_slice = env_u32("SLG_ROUNDS_PER_SLICE", 0);
  t->max_rounds_per_slice = env_u32("SLG_MAX_ROUNDS_PER_SLICE", 0);
  t->slices_per_subquery = env_u32("SLG_SLICES_PER_SUBQUERY", 16);
  t->cand_mode = 1;  // (reserved: k > 256 always runs on candidates + select)
  t->slice_order = env_i32("SLG_NO_SLICE_ORDER", 0) == 0;
  t->block_max = env_i32("SLG_NO_BLOCK_MAX", 0) == 0;
  t->pool_cap_mb = env_u32("SLG_POOL_CAP_MB", 0);
  t->uniform_kernel = env_u32("SLG_UNIFORM_KERNEL", 4);
  t->uniform_sigma_x100 = env_u32("SLG_UNIFORM_SIGMA", 0);
  t->inline_cuts = env_i32("SLG_INLINE_CUTS", -1);
  t->updatable = env_i32("SLG_NOT_UPDATABLE", 0) == 0;
  t->uniform_plans = env_i32("SLG_NO_UNIFORM_PLANS", 0) == 0;
  t->score_waves_per_simd = 0;  // (reserved: persistent scoring waves were removed)
}

slg_index *slg_index_create(const slg_segment_desc *segs, uint32_t n_segs, int device) {
  return slg_index_create_tuned(segs, n_segs, device, nullptr);
}

slg_index *slg_index_create_tuned(const slg_segment_desc *segs, uint32_t n_segs, int device,
                                  const slg_tuning *tuning) {
  slg_index *ix = nullptr;
  int rc = guarded([&] {
    SLG_REQUIRE(segs != nullptr && n_segs >= 1, "segs is NULL or n_segs == 0");
    slg_tuning tune;
    if (tuning) {
      SLG_REQUIRE(tuning->struct_size == sizeof(slg_tuning), "slg_tuning.struct_size mismatch");
      tune = *tuning;
    } else {
      slg_tuning_default(&tune);
    }
    // (4 is the only form left; a zero-initialised struct from a C or Rust caller is rejected here)
    if (tune.uniform_kernel == 2 || tune.uniform_kernel == 3)
      throw SlgError(SLG_ERR_UNSUPPORTED, "slg_tuning.uniform_kernel 2 / 3: those forms of the few-term kernel were removed");
    SLG_REQUIRE(tune.uniform_kernel == 4, "slg_tuning.uniform_kernel must be 4");
    if (tune.score_waves_per_simd != 0)
      throw SlgError(SLG_ERR_UNSUPPORTED, "slg_tuning.score_waves_per_simd must be 0: persistent scoring waves were removed");
    if (tune.cand_mode != 1)
      throw SlgError(SLG_ERR_UNSUPPORTED, "slg_tuning.cand_mode must be 1: 256 < k <= 1024 has no register top-k path");
    tune.uniform_max_terms = std::min<uint32_t>(tune.uniform_max_terms, slg::kU4MaxLists);
    tune.max_rounds_per_slice = std::min<uint32_t>(tune.max_rounds_per_slice, slg::kMaxRoundsPerSlice);
    tune.slices_per_subquery = std::max<uint32_t>(1, tune.slices_per_subquery);
    for (uint32_t s = 0; s < n_segs; s++) validate_segment(segs[s], s, tune.validate != 0);
    int ndev = 0;
    SLG_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)
      throw SlgError(SLG_ERR_DEVICE, "no such HIP device " + std::to_string(device));
    ix = new slg_index();
    ix->tune = tune;
    ix->device = device;
    DeviceGuard g(device);
    hipDeviceProp_t prop;
    SLG_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0 && !tune.allow_any_arch)
      throw SlgError(SLG_ERR_DEVICE,
                     std::string("device is ") + prop.gcnArchName + ", this library targets gfx950");
    SLG_HIP(hipStreamCreateWithFlags(&ix->own_stream, hipStreamNonBlocking));
    ix->stream = ix->own_stream;
    for (auto &us : ix->upload_streams) SLG_HIP(hipStreamCreateWithFlags(&us, hipStreamNonBlocking));
    auto st0 = std::make_unique<IndexState>();
    st0->generation = 0;
    st0->device = device;
    for (uint32_t s = 0; s < n_segs; s++) st0->segs.push_back(stage_segment(ix, segs[s]));
    {  // bound of the work-buffer pool (BufPool): a quarter of what staging left free
      size_t cap = (size_t)tune.pool_cap_mb << 20;
      if (tune.pool_cap_mb == 0) {
        size_t free_b = 0, total_b = 0;
        SLG_HIP(hipMemGetInfo(&free_b, &total_b));
        cap = std::min<size_t>(24ull << 30, std::max<size_t>(1ull << 30, free_b / 4));
        ix->tune.pool_cap_mb = (uint32_t)(cap >> 20);
      }
      ix->pool.cap = cap;
    }
    ix->d_error_flag.alloc(16, &ix->pool);
    SLG_HIP(hipMemset(ix->d_error_flag.p, 0, 16));
    finish_state(ix, *st0);
    publish(ix, std::move(st0));
  });
  if (rc != SLG_OK) {
    KeepLastError keep;
    if (ix) slg_index_destroy(ix);
    return nullptr;
  }
  return ix;
}

void slg_index_destroy(slg_index *ix) {
  if (!ix) return;
  DeviceScope on(ix->device);
  (void)hipDeviceSynchronize();  // batches may run on streams of their own
  {
    // batches that outlive the index are detached: buffers freed, handle stays valid for
    // slg_batch_destroy, every other call on it fails with SLG_ERR_INVALID
    std::lock_guard<std::mutex> lk(ix->mu);
    for (slg_batch *b : ix->live) {
      release_batch_buffers(b);
      b->snap.reset();
      b->idx = nullptr;
    }
    ix->live.clear();
  }
  for (auto &pr : ix->prof_events) {
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  {
    std::shared_ptr<const IndexState> last;
    std::lock_guard<std::mutex> lk(ix->mu);
    last.swap(ix->state);
  }  // (the state's device memory goes here unless a detached batch handle still holds a snapshot)
  ix->d_error_flag.release();
  if (ix->own_stream) (void)hipStreamDestroy(ix->own_stream);
  for (auto us : ix->upload_streams)
    if (us) (void)hipStreamDestroy(us);
  delete ix;
}

int slg_index_get_tuning(const slg_index *ix, slg_tuning *out) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr && out != nullptr, "index or out is NULL");
    *out = ix->tune;
  });
}

int slg_index_trim_pool(slg_index *ix, uint64_t *freed_bytes) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    DeviceGuard g(ix->device);
    const size_t freed = ix->pool.drain();
    if (freed_bytes) *freed_bytes = freed;
  });
}

int slg_index_info(const slg_index *ix, uint32_t *n_segs, uint64_t *n_postings,
                   uint64_t *device_bytes) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    const auto st = const_cast<slg_index *>(ix)->snapshot();
    uint64_t P = 0;
    for (auto &s : st->segs) P += s->n_postings;
    if (n_segs) *n_segs = (uint32_t)st->segs.size();
    if (n_postings) *n_postings = P;
    if (device_bytes) *device_bytes = state_device_bytes(*st);
  });
}

int slg_index_fetch_champions(const slg_index *ix, uint32_t seg, float *out) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(out != nullptr, "out is NULL");
    const auto st = const_cast<slg_index *>(ix)->snapshot();
    SLG_REQUIRE(seg < st->segs.size(), "no such segment");
    if (!ix->tune.champions)
      throw SlgError(SLG_ERR_UNSUPPORTED, "index was created with slg_tuning.champions = 0");
    const SegHost &sh = *st->segs[seg];
    const size_t n = (size_t)sh.n_terms * slg::kChampions;
    if (sh.champ.size() == n)
      std::memcpy(out, sh.champ.data(), n * sizeof(float));
    else  // (a segment without postings stages no table)
      std::fill(out, out + n, 0.0f);
  });
}

int slg_index_set_stream(slg_index *ix, void *hip_stream) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard g(ix->device);
    SLG_HIP(hipStreamSynchronize(ix->stream));
    ix->stream = hip_stream == SLG_OWN_STREAM ? ix->own_stream : (hipStream_t)hip_stream;
  });
}


// ---- doc filters -------------------------------------------------------------
namespace {
int add_filter_impl(slg_index *ix, const uint8_t *const *seg_bitmaps, const void *const *seg_columns,
                    int column_kind, long long lo_i, long long hi_i, double lo_f, double hi_f,
                    const uint32_t *term_ids = nullptr, uint32_t n_terms = 0, int pass_if_absent = 0) {
  int id = -1;
  int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      hipStream_t st = ix->stream;
      const size_t n_segs = cur.segs.size();
      auto fd = std::make_shared<FilterData>();
      fd->per_seg.resize(n_segs);
      std::vector<DevBuf> tmp(n_segs);  // uploaded pass bitmaps / columns (freed on return)
      std::vector<DevBuf> marked(n_segs);  // docs that hold one of the terms (slg_index_add_filter_terms)
      SLG_REQUIRE(n_terms == 0 || term_ids != nullptr, "term_ids is NULL");
      for (size_t s = 0; s < n_segs; s++) {
        const SegHost &sh = *cur.segs[s];
        const size_t words = ((size_t)sh.n_docs + 31) / 32;
        fd->per_seg[s] = std::make_shared<DevBuf>();
        fd->per_seg[s]->alloc((words ? words : 1) * 4, &ix->pool);
        slg::FilterBuildParams fp{};
        fp.deleted = sh.d_deleted.as<uint32_t>();
        fp.n_docs = sh.n_docs;
        fp.reject = fd->per_seg[s]->as<uint32_t>();
        fp.column_kind = 0;
        if (column_kind) {
          SLG_REQUIRE(seg_columns && seg_columns[s], "filter column of a segment is NULL");
          tmp[s].alloc((size_t)std::max<uint32_t>(sh.n_docs, 1) * 8, &ix->pool);
          SLG_HIP(hipMemcpyAsync(tmp[s].p, seg_columns[s], (size_t)sh.n_docs * 8, hipMemcpyHostToDevice, st));
          fp.column = tmp[s].p;
          fp.column_kind = column_kind;
          fp.lo_i = lo_i;
          fp.hi_i = hi_i;
          fp.lo_f = lo_f;
          fp.hi_f = hi_f;
        } else if (seg_bitmaps && seg_bitmaps[s]) {
          std::vector<uint32_t> w(words ? words : 1, 0u);
          std::memcpy(w.data(), seg_bitmaps[s], ((size_t)sh.n_docs + 7) / 8);
          tmp[s].alloc(w.size() * 4, &ix->pool);
          SLG_HIP(hipMemcpy(tmp[s].p, w.data(), w.size() * 4, hipMemcpyHostToDevice));
          fp.pass = tmp[s].as<uint32_t>();
        }
        if (term_ids) {
          // the docs of the given posting lists, marked on the device (the lists are resident: nothing is
          // uploaded but a bitmap's worth of zeros); a caller's bitmap, if any, is AND-ed as a second pass set
          const PostingStore &ps = *sh.store;
          marked[s].alloc((words ? words : 1) * 4, &ix->pool);
          SLG_HIP(hipMemsetAsync(marked[s].p, 0, (words ? words : 1) * 4, st));
          for (uint32_t t = 0; t < n_terms; t++) {
            const uint32_t id = term_ids[(size_t)t * n_segs + s];
            if (id == SLG_NO_TERM) continue;
            SLG_REQUIRE(id < ps.n_terms, "term id out of range");
            const uint64_t a = ps.term_offsets[id], b = ps.term_offsets[(size_t)id + 1];
            if (b == a || sh.n_docs == 0) continue;
            slg::PostingMarkParams mp{};
            mp.docs = ps.d_docs.as<uint32_t>() + a + (uint64_t)slg::kListPad * id;
            mp.df = (uint32_t)(b - a);
            mp.n_docs = sh.n_docs;
            mp.bitmap = marked[s].as<uint32_t>();
            hipLaunchKernelGGL(slg::posting_mark_kernel, dim3((mp.df + 255) / 256), dim3(256), 0, st, mp);
            SLG_HIP(hipGetLastError());
          }
          fp.pass2 = fp.pass;  // (the caller's bitmap, or nullptr)
          fp.pass = marked[s].as<uint32_t>();
          fp.invert_pass = pass_if_absent ? 1 : 0;
        }
        if (sh.n_docs) {
          hipLaunchKernelGGL(slg::filter_build_kernel, dim3((sh.n_docs + 255) / 256), dim3(256), 0, st, fp);
          SLG_HIP(hipGetLastError());
        }
      }
      SLG_HIP(hipStreamSynchronize(st));
      // the filter takes the lowest free id (ids of removed filters are reused, so the pointer table stays
      // as small as the number of filters alive at once)
      size_t slot = 0;
      while (slot < ns.filters.size() && ns.filters[slot]) slot++;
      if (slot == ns.filters.size()) ns.filters.emplace_back();
      ns.filters[slot] = std::move(fd);
      id = (int)slot;
    });
  });
  return rc == SLG_OK ? id : rc;
}
}  // namespace

int slg_index_add_filter(slg_index *ix, const uint8_t *const *seg_bitmaps) {
  return add_filter_impl(ix, seg_bitmaps, nullptr, 0, 0, 0, 0.0, 0.0);
}
int slg_index_add_filter_range_i64(slg_index *ix, const int64_t *const *seg_columns, int64_t lo, int64_t hi) {
  return add_filter_impl(ix, nullptr, reinterpret_cast<const void *const *>(seg_columns), 1, lo, hi, 0.0, 0.0);
}
int slg_index_add_filter_range_f64(slg_index *ix, const double *const *seg_columns, double lo, double hi) {
  return add_filter_impl(ix, nullptr, reinterpret_cast<const void *const *>(seg_columns), 2, 0, 0, lo, hi);
}
int slg_index_add_filter_terms(slg_index *ix, const uint32_t *term_ids, uint32_t n_terms, int pass_if_absent,
                               const uint8_t *const *and_bitmaps_or_null) {
  if (!term_ids && n_terms) {
    return guarded([&] { SLG_REQUIRE(false, "term_ids is NULL"); });
  }
  static const uint32_t none = SLG_NO_TERM;
  return add_filter_impl(ix, and_bitmaps_or_null, nullptr, 0, 0, 0, 0.0, 0.0, term_ids ? term_ids : &none, n_terms,
                         pass_if_absent);
}
int slg_index_remove_filter(slg_index *ix, int filter_id) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      SLG_REQUIRE(filter_id >= 0 && (size_t)filter_id < cur.filters.size() && cur.filters[filter_id],
                  "unknown filter id");
      // batches prepared with the filter hold the state that owns its bitmaps and its table row: they
      // may still run.  The slot is free for the next add
      ns.filters[filter_id].reset();
      while (!ns.filters.empty() && !ns.filters.back()) ns.filters.pop_back();
    });
  });
}

// ---- filter trees built on the device (slg_filter.hpp; the checks and the image: slg_plan.cpp) ----
int slg_index_add_filter_trees(slg_index *ix, const slg_filter_tree *trees, uint32_t n_trees, int32_t *out_ids) {
  return guarded([&] {
    slgplan::check_filter_trees(trees, n_trees);  // (host only, before the index is looked at)
    SLG_REQUIRE(out_ids != nullptr, "out_ids is NULL");
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    std::vector<int32_t> ids(n_trees, -1);  // (handed out only once the state is published: all or nothing)
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      hipStream_t st = ix->stream;
      const size_t n_segs = cur.segs.size();
      std::vector<char> live(cur.filters.size());
      for (size_t f = 0; f < live.size(); f++) live[f] = cur.filter_usable(f) ? 1 : 0;
      slgplan::FilterTreePlan fp;
      slgplan::plan_filter_trees(fscore_field_views(cur), cur.reject_host.data(), live.data(), live.size(),
                                 (uint32_t)n_segs, trees, n_trees, fp);
      // the new filters' bitmaps, and their addresses as the image's last table
      std::vector<std::shared_ptr<FilterData>> made(n_trees);
      std::vector<uint32_t *> outs((size_t)n_trees * n_segs);
      for (uint32_t t = 0; t < n_trees; t++) {
        made[t] = std::make_shared<FilterData>();
        made[t]->per_seg.resize(n_segs);
        for (size_t s = 0; s < n_segs; s++) {
          const size_t words = ((size_t)cur.segs[s]->n_docs + 31) / 32;
          made[t]->per_seg[s] = std::make_shared<DevBuf>();
          made[t]->per_seg[s]->alloc((words ? words : 1) * 4, &ix->pool);
          outs[(size_t)t * n_segs + s] = made[t]->per_seg[s]->as<uint32_t>();
        }
      }
      DevBuf image;  // one pooled upload (freed on return: the stream is synchronised below)
      upload_image(image, &ix->pool, {image_part(fp.trees), image_part(fp.nodes), image_part(fp.cols),
                                      image_part(fp.filters), image_part(outs), image_part(fp.words)});
      slg::FilterTreeParams p{};
      unsigned char *base = image.as<unsigned char>();
      p.trees = reinterpret_cast<const slg::FilterTreeDev *>(base);
      base += fp.trees.size() * sizeof(slg::FilterTreeDev);
      p.nodes = reinterpret_cast<const slg::FilterNodeDev *>(base);
      base += fp.nodes.size() * sizeof(slg::FilterNodeDev);
      p.cols = reinterpret_cast<const slg::ColumnDev *>(base);
      base += fp.cols.size() * sizeof(slg::ColumnDev);
      p.filters = reinterpret_cast<const uint32_t *const *>(base);
      base += fp.filters.size() * sizeof(void *);
      p.out = reinterpret_cast<uint32_t *const *>(base);
      base += outs.size() * sizeof(void *);
      p.words = reinterpret_cast<const uint32_t *>(base);
      p.n_segs = (uint32_t)n_segs;
      for (size_t s = 0; s < n_segs; s++) {
        const SegHost &sh = *cur.segs[s];
        if (sh.n_docs == 0) continue;
        p.deleted = sh.d_deleted.as<uint32_t>();
        p.n_docs = sh.n_docs;
        p.seg = (uint32_t)s;
        hipLaunchKernelGGL(slg::filter_tree_kernel, dim3((sh.n_docs + slg::kFilterThreads - 1) / slg::kFilterThreads, n_trees),
                           dim3(slg::kFilterThreads), 0, st, p);
        SLG_HIP(hipGetLastError());
      }
      SLG_HIP(hipStreamSynchronize(st));
      // every filter takes the lowest free id, in the order of the trees (add_filter_impl's policy)
      size_t slot = 0;
      for (uint32_t t = 0; t < n_trees; t++) {
        while (slot < ns.filters.size() && ns.filters[slot]) slot++;
        if (slot == ns.filters.size()) ns.filters.emplace_back();
        ns.filters[slot] = std::move(made[t]);
        ids[t] = (int32_t)slot;
      }
    });
    std::copy(ids.begin(), ids.end(), out_ids);
  });
}

// ---- nested paths, nested value columns and the trees over them (slg_nested.hpp; planner: slg_plan.cpp) ----
namespace {
void stage_words(slg_index *ix, DevBuf &dst, const uint32_t *src, size_t n) {
  dst.alloc(std::max<size_t>(n, 1) * 4, &ix->pool);
  if (n) SLG_HIP(hipMemcpy(dst.p, src, n * 4, hipMemcpyHostToDevice));
}
// offs[0 .. n] must not decrease -> offs[n] - offs[0]
size_t checked_span(const uint32_t *offs, size_t n, const char *what) {
  for (size_t i = 0; i < n; i++) SLG_REQUIRE(offs[i + 1] >= offs[i], what);
  return (size_t)offs[n] - offs[0];
}
void rebase(const uint32_t *offs, size_t n, std::vector<uint32_t> &o) {
  o.resize(n + 1);
  for (size_t i = 0; i <= n; i++) o[i] = offs[i] - offs[0];
}

// kind: 1 f64 values, 2 i64 values (kept as int64), 3 u32 ordinals
int add_nested_field_impl(slg_index *ix, int kind, int path_id, const uint32_t *const *seg_doc_offsets,
                          const uint32_t *const *seg_object_offsets, const void *const *seg_values, uint32_t n_ords) {
  int id = -1;
  const int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(seg_doc_offsets != nullptr, "seg_doc_offsets is NULL");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      SLG_REQUIRE(cur.nested_paths.count(path_id) == 1, "unknown nested path id");
      const size_t n_segs = cur.segs.size();
      auto fd = std::make_shared<NestedFieldData>();
      fd->path = path_id;
      fd->kind = kind;
      fd->n_ords = n_ords;
      fd->per_seg.resize(n_segs);
      const size_t width = kind == 3 ? 4 : 8;
      for (size_t s = 0; s < n_segs; s++) {
        const uint32_t n_docs = cur.segs[s]->n_docs;
        auto col = std::make_shared<NestedColSeg>();
        if (const uint32_t *doffs = seg_doc_offsets[s]) {
          const size_t n_obj = checked_span(doffs, n_docs, "nested field doc offsets of a segment are not monotone");
          SLG_REQUIRE(seg_object_offsets != nullptr && seg_object_offsets[s] != nullptr,
                      "nested field object offsets of a segment are NULL");
          const uint32_t *ooffs = seg_object_offsets[s] + doffs[0];
          const size_t nv = checked_span(ooffs, n_obj, "nested field object offsets of a segment are not monotone");
          SLG_REQUIRE(nv == 0 || (seg_values != nullptr && seg_values[s] != nullptr), "nested field values of a segment are NULL");
          const unsigned char *v = nv ? static_cast<const unsigned char *>(seg_values[s]) + (size_t)ooffs[0] * width : nullptr;
          if (kind == 3)
            for (size_t i = 0; i < nv; i++)
              SLG_REQUIRE(reinterpret_cast<const uint32_t *>(v)[i] < n_ords, "keyword ordinal >= n_ords");
          std::vector<uint32_t> d, o;
          rebase(doffs, n_docs, d);
          rebase(ooffs, n_obj, o);
          stage_words(ix, col->doc_offs, d.data(), d.size());
          stage_words(ix, col->obj_offs, o.data(), o.size());
          col->vals.alloc(std::max<size_t>(nv, 1) * width, &ix->pool);
          if (nv) SLG_HIP(hipMemcpy(col->vals.p, v, nv * width, hipMemcpyHostToDevice));
        }
        fd->per_seg[s] = std::move(col);
      }
      id = ix->next_nested_field++;
      ns.nested_fields.emplace(id, std::move(fd));
    });
  });
  return rc == SLG_OK ? id : rc;
}

// what the planner sees of the state's nested paths and nested fields (fscore_field_views' counterpart)
void nested_views(const IndexState &S, std::vector<slgplan::NestedPathView> &paths,
                  std::vector<slgplan::NestedFieldView> &fields) {
  for (const auto &kv : S.nested_paths) {
    slgplan::NestedPathView v;
    v.id = kv.first;
    v.parent = kv.second->parent;
    for (const auto &c : kv.second->per_seg) {
      slg::NestedPathDev d{};
      if (c) {
        d.base = c->base.as<uint32_t>();
        d.obj_doc = c->obj_doc.as<uint32_t>();
        d.par_offs = c->par_offs.p ? c->par_offs.as<uint32_t>() : nullptr;
        d.parents = c->parents.p ? c->parents.as<uint32_t>() : nullptr;
        d.n_objects = c->n_objects;
      }
      v.per_seg.push_back(d);
    }
    paths.push_back(std::move(v));
  }
  for (const auto &kv : S.nested_fields) {
    slgplan::NestedFieldView v;
    v.id = kv.first;
    v.path = kv.second->path;
    v.kind = kv.second->kind;
    v.n_ords = kv.second->n_ords;
    for (const auto &c : kv.second->per_seg) {
      slg::NestedColDev d{};
      if (c && c->doc_offs.p) {
        d.doc_offs = c->doc_offs.as<uint32_t>();
        d.obj_offs = c->obj_offs.as<uint32_t>();
        d.vals = c->vals.p;
      }
      v.per_seg.push_back(d);
      v.has.push_back(c ? 1 : 0);
    }
    fields.push_back(std::move(v));
  }
}
}  // namespace

int slg_index_add_nested_path(slg_index *ix, int parent_path_id, const uint32_t *const *seg_counts,
                              const uint32_t *const *seg_parent_offsets, const uint32_t *const *seg_parents) {
  int id = -1;
  const int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(parent_path_id >= -1, "parent_path_id below -1");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      SLG_REQUIRE(parent_path_id == -1 || cur.nested_paths.count(parent_path_id) == 1, "unknown parent nested path id");
      const size_t n_segs = cur.segs.size();
      auto pd = std::make_shared<NestedPathData>();
      pd->parent = parent_path_id;
      pd->per_seg.resize(n_segs);
      for (size_t s = 0; s < n_segs; s++) {
        const uint32_t n_docs = cur.segs[s]->n_docs;
        const uint32_t *counts = seg_counts ? seg_counts[s] : nullptr;
        // the docs' first objects: the prefix sum of the counts (u32 on the device, as every offset of the file)
        std::vector<uint32_t> base((size_t)n_docs + 1, 0u);
        uint64_t total = 0;
        for (uint32_t d = 0; d < n_docs; d++) {
          base[d] = (uint32_t)total;
          total += counts ? counts[d] : 0u;
          if (total > 0xFFFFFFFFull)
            throw SlgError(SLG_ERR_UNSUPPORTED, "a segment holds more than 2^32 - 1 objects of the nested path");
        }
        base[n_docs] = (uint32_t)total;
        std::vector<uint32_t> obj_doc((size_t)total);
        for (uint32_t d = 0; d < n_docs; d++) std::fill(obj_doc.begin() + base[d], obj_doc.begin() + base[d + 1], d);
        auto seg = std::make_shared<NestedPathSeg>();
        seg->n_objects = (uint32_t)total;
        stage_words(ix, seg->base, base.data(), base.size());
        stage_words(ix, seg->obj_doc, obj_doc.data(), obj_doc.size());
        if (const uint32_t *poffs = seg_parent_offsets ? seg_parent_offsets[s] : nullptr) {
          const size_t np = checked_span(poffs, n_docs, "nested parent offsets of a segment are not monotone");
          SLG_REQUIRE(np == 0 || (seg_parents != nullptr && seg_parents[s] != nullptr), "nested parents of a segment are NULL");
          std::vector<uint32_t> o;
          rebase(poffs, n_docs, o);
          stage_words(ix, seg->par_offs, o.data(), o.size());
          stage_words(ix, seg->parents, np ? seg_parents[s] + poffs[0] : nullptr, np);
        }
        pd->per_seg[s] = std::move(seg);
      }
      id = ix->next_nested_path++;
      ns.nested_paths.emplace(id, std::move(pd));
    });
  });
  return rc == SLG_OK ? id : rc;
}
int slg_index_remove_nested_path(slg_index *ix, int path_id) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      SLG_REQUIRE(cur.nested_paths.count(path_id) == 1, "unknown nested path id");
      ns.nested_paths.erase(path_id);
      for (auto it = ns.nested_fields.begin(); it != ns.nested_fields.end();)
        it = it->second->path == path_id ? ns.nested_fields.erase(it) : std::next(it);
    });
  });
}
int slg_index_add_nested_field_f64(slg_index *ix, int path_id, const uint32_t *const *seg_doc_offsets,
                                   const uint32_t *const *seg_object_offsets, const double *const *seg_values) {
  return add_nested_field_impl(ix, 1, path_id, seg_doc_offsets, seg_object_offsets,
                               reinterpret_cast<const void *const *>(seg_values), 0);
}
int slg_index_add_nested_field_i64(slg_index *ix, int path_id, const uint32_t *const *seg_doc_offsets,
                                   const uint32_t *const *seg_object_offsets, const int64_t *const *seg_values) {
  return add_nested_field_impl(ix, 2, path_id, seg_doc_offsets, seg_object_offsets,
                               reinterpret_cast<const void *const *>(seg_values), 0);
}
int slg_index_add_nested_field_ord(slg_index *ix, int path_id, const uint32_t *const *seg_doc_offsets,
                                   const uint32_t *const *seg_object_offsets, const uint32_t *const *seg_ords,
                                   uint32_t n_ords) {
  return add_nested_field_impl(ix, 3, path_id, seg_doc_offsets, seg_object_offsets,
                               reinterpret_cast<const void *const *>(seg_ords), n_ords);
}
int slg_index_remove_nested_field(slg_index *ix, int nested_field_id) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      SLG_REQUIRE(cur.nested_fields.count(nested_field_id) == 1, "unknown nested field id");
      ns.nested_fields.erase(nested_field_id);
    });
  });
}

int slg_index_add_nested_filter_trees(slg_index *ix, const slg_nested_filter_tree *trees, uint32_t n_trees,
                                      int32_t *out_ids) {
  return guarded([&] {
    slgplan::check_nested_filter_trees(trees, n_trees);  // (host only, before the index is looked at)
    SLG_REQUIRE(out_ids != nullptr, "out_ids is NULL");
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    std::vector<int32_t> ids(n_trees, -1);  // (handed out only once the state is published: all or nothing)
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      hipStream_t st = ix->stream;
      const size_t n_segs = cur.segs.size();
      std::vector<char> live(cur.filters.size());
      for (size_t f = 0; f < live.size(); f++) live[f] = cur.filter_usable(f) ? 1 : 0;
      std::vector<slgplan::NestedPathView> paths;
      std::vector<slgplan::NestedFieldView> nfields;
      nested_views(cur, paths, nfields);
      slgplan::NestedFilterPlan np;
      slgplan::plan_nested_filter_trees(fscore_field_views(cur), cur.reject_host.data(), live.data(), live.size(), paths,
                                        nfields, (uint32_t)n_segs, trees, n_trees, np);
      // the new filters' bitmaps, and the object scopes' transient ones (pooled: back on return, the stream is
      // synchronised below); their addresses are two tables of the image
      std::vector<std::shared_ptr<FilterData>> made(n_trees);
      std::vector<uint32_t *> outs((size_t)n_trees * n_segs);
      for (uint32_t t = 0; t < n_trees; t++) {
        made[t] = std::make_shared<FilterData>();
        made[t]->per_seg.resize(n_segs);
        for (size_t s = 0; s < n_segs; s++) {
          const size_t words = ((size_t)cur.segs[s]->n_docs + 31) / 32;
          made[t]->per_seg[s] = std::make_shared<DevBuf>();
          made[t]->per_seg[s]->alloc((words ? words : 1) * 4, &ix->pool);
          outs[(size_t)t * n_segs + s] = made[t]->per_seg[s]->as<uint32_t>();
        }
      }
      const uint32_t n_obj_scopes = np.level_begin.back();
      const auto n_objects = [&](uint32_t row, size_t s) { return np.paths[(size_t)np.scopes[row].path_row * n_segs + s].n_objects; };
      std::vector<DevBuf> bits((size_t)n_obj_scopes * n_segs);
      std::vector<uint32_t *> obj_bits(bits.size());
      for (uint32_t r = 0; r < n_obj_scopes; r++)
        for (size_t s = 0; s < n_segs; s++) {
          DevBuf &b = bits[(size_t)r * n_segs + s];
          b.alloc_pooled(&ix->pool, std::max<size_t>(((size_t)n_objects(r, s) + 31) / 32, 1) * 4);
          obj_bits[(size_t)r * n_segs + s] = b.as<uint32_t>();
        }
      DevBuf image;
      upload_image(image, &ix->pool, {image_part(np.scopes), image_part(np.nodes), image_part(np.cols),
                                      image_part(np.filters), image_part(np.paths), image_part(np.ncols),
                                      image_part(obj_bits), image_part(outs), image_part(np.words)});
      slg::NestedFilterParams p{};
      unsigned char *base = image.as<unsigned char>();
      const auto take = [&base](auto *&dst, size_t bytes) {
        dst = reinterpret_cast<std::remove_reference_t<decltype(dst)>>(base);
        base += bytes;
      };
      take(p.scopes, np.scopes.size() * sizeof(slg::NestedScopeDev));
      take(p.nodes, np.nodes.size() * sizeof(slg::FilterNodeDev));
      take(p.cols, np.cols.size() * sizeof(slg::ColumnDev));
      take(p.filters, np.filters.size() * sizeof(void *));
      take(p.paths, np.paths.size() * sizeof(slg::NestedPathDev));
      take(p.ncols, np.ncols.size() * sizeof(slg::NestedColDev));
      take(p.obj_bits, obj_bits.size() * sizeof(void *));
      take(p.out, outs.size() * sizeof(void *));
      take(p.words, np.words.size() * 4);
      p.n_segs = (uint32_t)n_segs;
      // level by level, the deepest object scopes first: (levels + 1) launches per segment, a level's scopes of
      // every tree on blockIdx.y
      for (size_t s = 0; s < n_segs; s++) {
        const SegHost &sh = *cur.segs[s];
        if (sh.n_docs == 0) continue;
        p.deleted = sh.d_deleted.as<uint32_t>();
        p.n_docs = sh.n_docs;
        p.seg = (uint32_t)s;
        for (size_t l = 0; l + 1 < np.level_begin.size(); l++) {
          p.first_scope = np.level_begin[l];
          const uint32_t n_scopes = np.level_begin[l + 1] - p.first_scope;
          uint32_t most = 0;
          for (uint32_t r = 0; r < n_scopes; r++) most = std::max(most, n_objects(p.first_scope + r, s));
          if (most == 0) continue;  // (no object: the bitmaps of this level are never read in this segment)
          hipLaunchKernelGGL(slg::nested_filter_kernel<false>,
                             dim3((uint32_t)(((uint64_t)most + slg::kFilterThreads - 1) / slg::kFilterThreads), n_scopes),
                             dim3(slg::kFilterThreads), 0, st, p);
          SLG_HIP(hipGetLastError());
        }
        p.first_scope = n_obj_scopes;
        hipLaunchKernelGGL(slg::nested_filter_kernel<true>, dim3((sh.n_docs + slg::kFilterThreads - 1) / slg::kFilterThreads, n_trees),
                           dim3(slg::kFilterThreads), 0, st, p);
        SLG_HIP(hipGetLastError());
      }
      SLG_HIP(hipStreamSynchronize(st));
      // every filter takes the lowest free id, in the order of the trees (add_filter_impl's policy)
      size_t slot = 0;
      for (uint32_t t = 0; t < n_trees; t++) {
        while (slot < ns.filters.size() && ns.filters[slot]) slot++;
        if (slot == ns.filters.size()) ns.filters.emplace_back();
        ns.filters[slot] = std::move(made[t]);
        ids[t] = (int32_t)slot;
      }
    });
    std::copy(ids.begin(), ids.end(), out_ids);
  });
}

int slg_index_fetch_filter(slg_index *ix, int filter_id, uint32_t seg, uint8_t *out_pass) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(out_pass != nullptr, "out_pass is NULL");
    const auto st = ix->snapshot();
    SLG_REQUIRE(filter_id >= 0 && (size_t)filter_id < st->filters.size() && st->filters[filter_id], "unknown filter id");
    SLG_REQUIRE(seg < st->segs.size(), "no such segment");
    const FilterData &fd = *st->filters[filter_id];
    SLG_REQUIRE(seg < fd.per_seg.size() && fd.per_seg[seg], "the filter has no bitmap for this segment (added after it was registered)");
    const uint32_t n_docs = st->segs[seg]->n_docs;
    const size_t words = ((size_t)n_docs + 31) / 32;
    if (words == 0) return;
    DeviceGuard g(ix->device);
    std::vector<uint32_t> w(words);
    SLG_HIP(hipMemcpy(w.data(), fd.per_seg[seg]->p, words * 4, hipMemcpyDeviceToHost));
    for (auto &x : w) x = ~x;  // (bits past n_docs are set in the reject bitmap: clear here)
    std::memcpy(out_pass, w.data(), ((size_t)n_docs + 7) / 8);
  });
}

// ---- sort fields (query/sort.rs:300-345) ---------------------------------------------------
namespace {
int add_sort_field_impl(slg_index *ix, int kind, const uint32_t *const *seg_offsets, const void *const *seg_values) {
  int id = -1;
  const int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(seg_offsets != nullptr, "seg_offsets is NULL");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      const size_t n_segs = cur.segs.size();
      auto fd = std::make_shared<SortFieldData>();
      fd->kind = kind;
      fd->per_seg.resize(n_segs);
      for (size_t s = 0; s < n_segs; s++) {
        const uint32_t n_docs = cur.segs[s]->n_docs;
        const uint32_t *offs = seg_offsets[s];
        SLG_REQUIRE(offs == nullptr || seg_values != nullptr, "seg_values is NULL");
        if (offs) {
          for (uint32_t d = 0; d < n_docs; d++)
            SLG_REQUIRE(offs[d + 1] >= offs[d], "sort field offsets of a segment are not monotone");
          SLG_REQUIRE(offs[n_docs] == offs[0] || seg_values[s] != nullptr, "sort field values of a segment are NULL");
        }
        // the Min / Max selection and the key encoding run on the host (slg_plan.cpp: unit-tested on the CPU)
        const size_t n = std::max<uint32_t>(n_docs, 1), words = (n + 31) / 32;
        std::vector<uint64_t> asc(n, 0), desc(n, 0);
        std::vector<uint32_t> present(words, 0);
        slgplan::sort_field_keys(kind, n_docs, offs, offs ? seg_values[s] : nullptr, asc.data(), desc.data(),
                                 present.data());
        auto col = std::make_shared<SortColumn>();
        col->key[0].alloc(n * 8, &ix->pool);
        col->key[1].alloc(n * 8, &ix->pool);
        col->present.alloc(words * 4, &ix->pool);
        SLG_HIP(hipMemcpy(col->key[0].p, asc.data(), n * 8, hipMemcpyHostToDevice));
        SLG_HIP(hipMemcpy(col->key[1].p, desc.data(), n * 8, hipMemcpyHostToDevice));
        SLG_HIP(hipMemcpy(col->present.p, present.data(), words * 4, hipMemcpyHostToDevice));
        fd->per_seg[s] = std::move(col);
      }
      id = ix->next_sort_field++;
      ns.sort_fields.emplace(id, std::move(fd));
    });
  });
  return rc == SLG_OK ? id : rc;
}
}  // namespace

int slg_index_add_sort_field_i64(slg_index *ix, const uint32_t *const *seg_offsets, const int64_t *const *seg_values) {
  return add_sort_field_impl(ix, 1, seg_offsets, reinterpret_cast<const void *const *>(seg_values));
}
int slg_index_add_sort_field_f64(slg_index *ix, const uint32_t *const *seg_offsets, const double *const *seg_values) {
  return add_sort_field_impl(ix, 2, seg_offsets, reinterpret_cast<const void *const *>(seg_values));
}
int slg_index_remove_sort_field(slg_index *ix, int sort_field_id) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      SLG_REQUIRE(cur.sort_fields.count(sort_field_id) == 1, "unknown sort field id");
      ns.sort_fields.erase(sort_field_id);
    });
  });
}

// ---- positions of a segment's postings (phrase queries; index/postings.rs:176-183) ---------------
int slg_index_set_positions(slg_index *ix, uint32_t seg, const uint64_t *pos_offsets, const uint32_t *positions) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      SLG_REQUIRE(seg < cur.segs.size(), "no such segment");
      ns.positions.resize(cur.segs.size());
      if (!pos_offsets && !positions) {  // the segment is back to keep_positions = false
        ns.positions[seg].reset();
        return;
      }
      const uint64_t P = cur.segs[seg]->n_postings;
      slgplan::check_positions(P, pos_offsets, positions);  // (host only, before any device work)
      const uint64_t total = pos_offsets[P];
      std::vector<uint32_t> offs(P + 1);
      for (uint64_t i = 0; i <= P; i++) offs[i] = (uint32_t)pos_offsets[i];
      auto store = std::make_shared<PosStore>();
      store->offs.alloc((P + 1) * 4, &ix->pool);
      store->pos.alloc(std::max<uint64_t>(total, 1) * 4, &ix->pool);
      SLG_HIP(hipMemcpy(store->offs.p, offs.data(), (P + 1) * 4, hipMemcpyHostToDevice));
      if (total) SLG_HIP(hipMemcpy(store->pos.p, positions, total * 4, hipMemcpyHostToDevice));
      ns.positions[seg] = std::move(store);
    });
  });
}

// ---- the term dictionary of a segment (term expansion; util/fst.rs:25-33) ------------------------
int slg_index_set_terms(slg_index *ix, uint32_t seg, const char *key_bytes, const uint32_t *key_offsets) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      SLG_REQUIRE(seg < cur.segs.size(), "no such segment");
      SLG_REQUIRE(key_bytes != nullptr, "set_terms: key_bytes is NULL");
      ns.terms.resize(cur.segs.size());
      auto store = std::make_shared<TermStore>();
      slgexpand::build_dict(cur.segs[seg]->n_terms, key_bytes, key_offsets, store->dict);  // (host only, before any device work)
      const slgexpand::Dict &d = store->dict;
      const auto stage = [&](DevBuf &b, const void *src, size_t bytes) {
        b.alloc(std::max<size_t>(bytes, 4), &ix->pool);
        if (bytes) SLG_HIP(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
      };
      stage(store->bytes, d.bytes.data(), d.bytes.size());
      stage(store->offs, d.offs.data(), d.offs.size() * 4);
      stage(store->map, d.map.data(), d.map.size() * 4);
      stage(store->nchars, d.nchars.data(), d.nchars.size());
      // the doc frequency of every key, in sorted-position order: the list lengths of the CSR as it was staged
      // (the PostingStore keeps the original term_offsets; tombstones never change them)
      const std::vector<uint64_t> &to = cur.segs[seg]->store->term_offsets;
      store->df.resize(d.n());
      store->nonzero.assign((size_t)d.n() + 1, 0u);
      for (uint32_t pos = 0; pos < d.n(); pos++) {
        store->df[pos] = (uint32_t)std::min<uint64_t>(to[d.map[pos] + 1] - to[d.map[pos]], 0xFFFFFFFFull);
        store->nonzero[pos + 1] = store->nonzero[pos] + (store->df[pos] != 0u);
      }
      stage(store->d_df, store->df.data(), store->df.size() * 4);
      ns.terms[seg] = std::move(store);
    });
  });
}

// ---- aggregation fields (query/aggs/mod.rs; index/fastfields.rs:711-800) -----------------------
namespace {
// kind: 1 f64 values, 2 i64 values (converted `as f64` here, as the reference does), 3 u32 ordinals
int add_agg_field_impl(slg_index *ix, int kind, const uint32_t *const *seg_offsets, const void *const *seg_values,
                       uint32_t n_ords) {
  int id = -1;
  const int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(seg_offsets != nullptr, "seg_offsets is NULL");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      const size_t n_segs = cur.segs.size();
      auto fd = std::make_shared<AggFieldData>();
      fd->kind = kind == 3 ? 2 : 1;
      fd->n_ords = n_ords;
      fd->from_i64 = kind == 2;
      fd->per_seg.resize(n_segs);
      fd->ranks.resize(n_segs);
      for (size_t s = 0; s < n_segs; s++) {
        const uint32_t n_docs = cur.segs[s]->n_docs;
        const uint32_t *offs = seg_offsets[s];
        SLG_REQUIRE(offs == nullptr || seg_values != nullptr, "seg_values is NULL");
        bool dense = offs != nullptr && n_docs > 0;
        if (offs) {
          for (uint32_t d = 0; d < n_docs; d++) {
            SLG_REQUIRE(offs[d + 1] >= offs[d], "agg field offsets of a segment are not monotone");
            dense = dense && offs[d] == offs[0] + d;
          }
          dense = dense && offs[n_docs] == offs[0] + n_docs;
          SLG_REQUIRE(offs[n_docs] == offs[0] || seg_values[s] != nullptr, "agg field values of a segment are NULL");
        }
        const uint32_t first = offs ? offs[0] : 0u;
        const size_t nv = offs ? (size_t)offs[n_docs] - first : 0;
        auto col = std::make_shared<AggColumn>();
        col->n_vals = nv;
        if (kind == 3) {
          const uint32_t *v = nv ? static_cast<const uint32_t *>(seg_values[s]) + first : nullptr;
          for (size_t i = 0; i < nv; i++) SLG_REQUIRE(v[i] < n_ords, "keyword ordinal >= n_ords");
          col->vals.alloc(std::max<size_t>(nv, 1) * 4, &ix->pool);
          if (nv) SLG_HIP(hipMemcpy(col->vals.p, v, nv * 4, hipMemcpyHostToDevice));
        } else {
          std::vector<double> conv;
          const double *v = nullptr;
          if (nv && kind == 2) {  // fastfields.rs:772-800: i64 values reach the collectors `as f64`
            const int64_t *iv = static_cast<const int64_t *>(seg_values[s]) + first;
            conv.resize(nv);
            constexpr int64_t i2p53 = (int64_t)1 << 53;
            for (size_t i = 0; i < nv; i++) {
              conv[i] = (double)iv[i];
              col->i64_rounded = col->i64_rounded || iv[i] > i2p53 || iv[i] < -i2p53;
            }
            v = conv.data();
          } else if (nv) {
            v = static_cast<const double *>(seg_values[s]) + first;
          }
          for (size_t i = 0; i < nv; i++) {
            if (!std::isfinite(v[i])) {
              col->non_finite = true;
              continue;
            }
            col->vmin = col->any_value ? std::min(col->vmin, v[i]) : v[i];
            col->vmax = col->any_value ? std::max(col->vmax, v[i]) : v[i];
            col->any_value = true;
          }
          col->vals.alloc(std::max<size_t>(nv, 1) * 8, &ix->pool);
          if (nv) SLG_HIP(hipMemcpy(col->vals.p, v, nv * 8, hipMemcpyHostToDevice));
        }
        if (!dense) {  // the offsets, rebased to the copied values (NULL: no doc has a value)
          std::vector<uint32_t> o((size_t)n_docs + 1, 0u);
          if (offs)
            for (uint32_t d = 0; d <= n_docs; d++) o[d] = offs[d] - first;
          col->offs.alloc(o.size() * 4, &ix->pool);
          SLG_HIP(hipMemcpy(col->offs.p, o.data(), o.size() * 4, hipMemcpyHostToDevice));
        }
        fd->per_seg[s] = std::move(col);
      }
      fd->refold();
      id = ix->next_agg_field++;
      ns.agg_fields.emplace(id, std::move(fd));
    });
  });
  return rc == SLG_OK ? id : rc;
}
}  // namespace

int slg_index_add_agg_field_f64(slg_index *ix, const uint32_t *const *seg_offsets, const double *const *seg_values) {
  return add_agg_field_impl(ix, 1, seg_offsets, reinterpret_cast<const void *const *>(seg_values), 0);
}
int slg_index_add_agg_field_i64(slg_index *ix, const uint32_t *const *seg_offsets, const int64_t *const *seg_values) {
  return add_agg_field_impl(ix, 2, seg_offsets, reinterpret_cast<const void *const *>(seg_values), 0);
}
int slg_index_add_agg_field_ord(slg_index *ix, const uint32_t *const *seg_offsets, const uint32_t *const *seg_ords,
                                uint32_t n_ords) {
  return add_agg_field_impl(ix, 3, seg_offsets, reinterpret_cast<const void *const *>(seg_ords), n_ords);
}
int64_t slg_index_rank_agg_field(slg_index *ix, int agg_field_id) {
  int64_t n_ranks = 0;
  const int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    // a keyword field's ordinals are its ranks; a ranked field stays as it is: no new state for either
    auto known = [&](const IndexState &S) {
      const auto it = S.agg_fields.find(agg_field_id);
      SLG_REQUIRE(it != S.agg_fields.end(), "unknown agg field id");
      if (it->second->kind == 2) n_ranks = it->second->n_ords;
      if (it->second->dict) n_ranks = (int64_t)it->second->dict->keys.size();
      return it->second->kind == 2 || it->second->dict != nullptr;
    };
    if (known(*ix->snapshot())) return;
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      if (known(cur)) return;  // (ranked by another thread in between)
      const AggFieldData &fd = *cur.agg_fields.find(agg_field_id)->second;
      if (fd.non_finite)
        throw SlgError(SLG_ERR_UNSUPPORTED, "agg field " + std::to_string(agg_field_id) + " holds a non-finite value");
      if (fd.i64_rounded)
        throw SlgError(SLG_ERR_UNSUPPORTED, "agg field " + std::to_string(agg_field_id) +
                                                " holds an i64 value beyond +-2^53: distinct values became one f64");
      auto key_of = [](double x) {  // = slg::agg_f64_key
        uint64_t b;
        std::memcpy(&b, &x, 8);
        return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
      };
      // the values come back from the device (registration kept no host copy); one sort over all of them
      std::vector<std::vector<uint64_t>> keys(fd.per_seg.size());
      auto dict = std::make_shared<AggRankDict>();
      for (size_t s = 0; s < fd.per_seg.size(); s++) {
        const auto &col = fd.per_seg[s];
        if (!col || col->n_vals == 0) continue;
        std::vector<double> v(col->n_vals);
        SLG_HIP(hipMemcpy(v.data(), col->vals.p, v.size() * 8, hipMemcpyDeviceToHost));
        keys[s].resize(v.size());
        for (size_t i = 0; i < v.size(); i++) keys[s][i] = key_of(v[i]);
        dict->keys.insert(dict->keys.end(), keys[s].begin(), keys[s].end());
      }
      std::sort(dict->keys.begin(), dict->keys.end());
      dict->keys.erase(std::unique(dict->keys.begin(), dict->keys.end()), dict->keys.end());
      dict->keys.shrink_to_fit();
      if (dict->keys.size() > SLG_MAX_AGG_RANKS)
        throw SlgError(SLG_ERR_UNSUPPORTED, "agg field " + std::to_string(agg_field_id) +
                                                " holds more than SLG_MAX_AGG_RANKS distinct values");
      auto nf = std::make_shared<AggFieldData>(fd);
      nf->ranks.assign(fd.per_seg.size(), nullptr);
      std::vector<uint32_t> r;
      for (size_t s = 0; s < fd.per_seg.size(); s++) {
        if (!fd.per_seg[s]) continue;
        r.resize(keys[s].size());
        for (size_t i = 0; i < r.size(); i++)
          r[i] = (uint32_t)(std::lower_bound(dict->keys.begin(), dict->keys.end(), keys[s][i]) - dict->keys.begin());
        auto buf = std::make_shared<DevBuf>();
        buf->alloc(std::max<size_t>(r.size(), 1) * 4, &ix->pool);
        if (!r.empty()) SLG_HIP(hipMemcpy(buf->p, r.data(), r.size() * 4, hipMemcpyHostToDevice));
        nf->ranks[s] = std::move(buf);
      }
      std::vector<double> vals(dict->keys.size());
      for (size_t i = 0; i < vals.size(); i++) {
        const uint64_t k = dict->keys[i], b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
        std::memcpy(&vals[i], &b, 8);
      }
      dict->vals.alloc(std::max<size_t>(vals.size(), 1) * 8, &ix->pool);
      if (!vals.empty()) SLG_HIP(hipMemcpy(dict->vals.p, vals.data(), vals.size() * 8, hipMemcpyHostToDevice));
      n_ranks = (int64_t)dict->keys.size();
      nf->dict = std::move(dict);
      ns.agg_fields[agg_field_id] = std::move(nf);
    });
  });
  return rc == SLG_OK ? n_ranks : rc;
}
int slg_index_remove_agg_field(slg_index *ix, int agg_field_id) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      SLG_REQUIRE(cur.agg_fields.count(agg_field_id) == 1, "unknown agg field id");
      ns.agg_fields.erase(agg_field_id);
    });
  });
}

// ---- text fields (slg_highlight_batch; index/highlight.rs, api/reader.rs:3400-3497) --------------
int slg_index_add_text_field(slg_index *ix, const uint64_t *const *seg_offsets, const uint8_t *const *seg_bytes) {
  int id = -1;
  const int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(seg_offsets != nullptr, "seg_offsets is NULL");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      const size_t n_segs = cur.segs.size();
      auto tf = std::make_shared<TextFieldHost>();
      tf->per_seg.resize(n_segs);
      for (size_t s = 0; s < n_segs; s++) {
        const uint64_t *offs = seg_offsets[s];
        if (!offs) continue;  // the segment has no text in the field
        const uint32_t n_docs = cur.segs[s]->n_docs;
        const uint64_t first = offs[0], total = offs[n_docs] - offs[0];
        for (uint32_t d = 0; d < n_docs; d++) {
          SLG_REQUIRE(offs[d + 1] >= offs[d], "text field offsets of a segment decrease");
          if (offs[d + 1] - offs[d] >= (1ull << 31)) throw SlgError(SLG_ERR_UNSUPPORTED, "a text of 2^31 bytes or more");
        }
        SLG_REQUIRE(total == 0 || (seg_bytes != nullptr && seg_bytes[s] != nullptr), "text field bytes of a segment are NULL");
        const uint8_t *src = total ? seg_bytes[s] + first : nullptr;
        std::vector<uint64_t> o((size_t)n_docs + 1);
        std::vector<uint32_t> bits(((size_t)n_docs + 31) / 32 + 1, 0u);
        for (uint32_t d = 0; d <= n_docs; d++) o[d] = offs[d] - first;
        for (uint32_t d = 0; d < n_docs; d++)
          for (uint64_t i = o[d]; i < o[d + 1]; i++)
            if (src[i] >= 0x80u) {
              bits[d >> 5] |= 1u << (d & 31u);
              break;
            }
        auto store = std::make_shared<TextSegStore>();
        store->n_docs = n_docs;
        // padded: the 16-byte line that holds a doc's last byte lies inside the allocation (whose start is aligned)
        store->bytes.alloc((size_t)total + 16, &ix->pool);
        SLG_HIP(hipMemset(store->bytes.p, 0, (size_t)total + 16));
        if (total) SLG_HIP(hipMemcpy(store->bytes.p, src, (size_t)total, hipMemcpyHostToDevice));
        store->offs.alloc(o.size() * 8, &ix->pool);
        SLG_HIP(hipMemcpy(store->offs.p, o.data(), o.size() * 8, hipMemcpyHostToDevice));
        store->non_ascii.alloc(bits.size() * 4, &ix->pool);
        SLG_HIP(hipMemcpy(store->non_ascii.p, bits.data(), bits.size() * 4, hipMemcpyHostToDevice));
        tf->per_seg[s] = std::move(store);
      }
      id = ix->next_text_field++;
      ns.text_fields.emplace(id, std::move(tf));
    });
  });
  return rc == SLG_OK ? id : rc;
}
int slg_index_remove_text_field(slg_index *ix, int text_field_id) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      SLG_REQUIRE(cur.text_fields.count(text_field_id) == 1, "unknown text field id");
      ns.text_fields.erase(text_field_id);
    });
  });
}

// ---- index updates (api/writer.rs:106-240) ---------------------------------------------------
int slg_index_update_deleted(slg_index *ix, uint32_t seg, const uint8_t *deleted, float live_docs) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    update_state(ix, true, [&](const IndexState &cur, IndexState &ns) {
      SLG_REQUIRE(seg < cur.segs.size(), "no such segment");
      SLG_REQUIRE(live_docs >= 0.0f && live_docs <= (float)cur.segs[seg]->n_docs, "live_docs outside [0, n_docs]");
      const std::shared_ptr<PostingStore> &ps = cur.segs[seg]->store;
      if (!ps->updatable)
        throw SlgError(SLG_ERR_UNSUPPORTED, "index was created with slg_tuning.updatable = 0");
      auto sh = std::make_shared<SegHost>();
      derive_version(ix, ps, *sh, deleted, live_docs, StageTemps{});
      ns.segs[seg] = sh;
      // registered filters: reject = deleted | ~filter, so this segment's bitmaps take the new tombstones
      const size_t words = std::max<size_t>(((size_t)ps->n_docs + 31) / 32, 1);
      for (auto &f : ns.filters) {
        if (!f || seg >= f->per_seg.size() || !f->per_seg[seg]) continue;
        auto nf = std::make_shared<FilterData>(*f);
        auto nb = std::make_shared<DevBuf>();
        nb->alloc(words * 4, &ix->pool);
        slg::BitmapOrParams bp{};
        bp.a = f->per_seg[seg]->as<uint32_t>();
        bp.b = sh->d_deleted.as<uint32_t>();
        bp.out = nb->as<uint32_t>();
        bp.n_words = (uint32_t)words;
        hipLaunchKernelGGL(slg::bitmap_or_kernel, dim3((uint32_t)((words + 255) / 256)), dim3(256), 0, ix->stream, bp);
        SLG_HIP(hipGetLastError());
        nf->per_seg[seg] = std::move(nb);
        f = std::move(nf);
      }
      SLG_HIP(hipStreamSynchronize(ix->stream));
    });
  });
}

int slg_index_add_segment(slg_index *ix, const slg_segment_desc *seg) {
  int ord = -1;
  const int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr && seg != nullptr, "index or segment descriptor is NULL");
    validate_segment(*seg, 0, ix->tune.validate != 0);
    update_state(ix, true, [&](const IndexState &, IndexState &ns) {
      ns.segs.push_back(stage_segment(ix, *seg));
      // no bitmap / column / store for the new segment: a filter or sort field registered before is
      // unusable until it is registered again
      const size_t n_segs = ns.segs.size();
      reshape_per_segment(ns, [n_segs](auto &per_seg) { per_seg.resize(n_segs); });
      // ... but the new segment's own store (field 0) is quantised here when field 0 has a bf16 copy
      const PostingStore &ps = *ns.segs.back()->store;
      const auto c0 = ns.vcopies.find(0u);
      if (c0 != ns.vcopies.end() && ps.vec_dim)
        c0->second->per_seg[n_segs - 1] = vs_quantize_store(ix, ps.d_vec_values.as<float>(), ps.vec_rows, ps.vec_dim);
      ord = (int)n_segs - 1;
    });
  });
  return rc == SLG_OK ? ord : rc;
}

int slg_index_remove_segment(slg_index *ix, uint32_t seg) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    update_state(ix, true, [&](const IndexState &cur, IndexState &ns) {
      SLG_REQUIRE(seg < cur.segs.size(), "no such segment");
      SLG_REQUIRE(cur.segs.size() > 1, "the last segment of an index cannot be removed (add the replacement first)");
      ns.segs.erase(ns.segs.begin() + seg);
      reshape_per_segment(ns, [seg](auto &per_seg) {
        if (seg < per_seg.size()) per_seg.erase(per_seg.begin() + seg);
      });
    });
  });
}

int slg_index_device(const slg_index *ix) {
  if (!ix) {
    last_error().msg = "index is NULL";
    last_error().code = SLG_ERR_INVALID;
    return SLG_ERR_INVALID;
  }
  return ix->device;
}

uint64_t slg_index_generation(const slg_index *ix) {
  return ix ? ix->generation.load(std::memory_order_acquire) : 0;  // (no lock: callers poll it per request)
}

int slg_profile_enable(slg_index *ix, int on) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    ix->profile = on != 0;
  });
}

int slg_profile_read(slg_index *ix, uint32_t *n_launches, float *total_ms) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard g(ix->device);
    float sum = 0.0f;
    for (size_t i = 0; i < ix->prof_used; i++) {
      SLG_HIP(hipEventSynchronize(ix->prof_events[i].second));
      float ms = 0.0f;
      SLG_HIP(hipEventElapsedTime(&ms, ix->prof_events[i].first, ix->prof_events[i].second));
      sum += ms;
    }
    if (n_launches) *n_launches = (uint32_t)ix->prof_used;
    if (total_ms) *total_ms = sum;
    ix->prof_used = 0;
  });
}

int slg_index_add_vector_field(slg_index *ix, const slg_vector_field_desc *per_segment, uint32_t n_segs) {
  int id = 0;
  const int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr && per_segment != nullptr, "index or descriptors are NULL");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      SLG_REQUIRE(n_segs == cur.segs.size(), "one descriptor per segment of the index is required");
      auto vf = std::make_shared<VecFieldHost>();
      for (uint32_t s = 0; s < n_segs; s++) {
        const slg_vector_field_desc &d = per_segment[s];
        if (!d.vec_dim) continue;
        SLG_REQUIRE(d.vec_offsets != nullptr && (d.vec_rows == 0 || d.vec_values != nullptr), "vector arrays are NULL");
        SLG_REQUIRE(d.vec_metric == SLG_METRIC_COSINE || d.vec_metric == SLG_METRIC_L2, "unknown vector metric");
        SLG_REQUIRE(vf->dim == 0 || (vf->dim == d.vec_dim && vf->metric == d.vec_metric),
                    "segments disagree on the field's dimension or metric");
        vf->dim = d.vec_dim;
        vf->metric = d.vec_metric;
        const uint32_t nd = cur.segs[s]->n_docs;
        for (uint32_t i = 0; i < nd; i++)
          SLG_REQUIRE(d.vec_offsets[i] == SLG_NO_VECTOR || d.vec_offsets[i] < d.vec_rows,
                      "vector offset past vec_rows");
      }
      SLG_REQUIRE(vf->dim != 0, "no segment has vectors in this field");
      vf->per_seg.resize(n_segs);
      for (uint32_t s = 0; s < n_segs; s++) {
        const slg_vector_field_desc &d = per_segment[s];
        if (!d.vec_dim) continue;
        auto vs = std::make_shared<VecSegStore>();
        const size_t ob = (size_t)cur.segs[s]->n_docs * 4, vb = (size_t)d.vec_rows * d.vec_dim * 4;
        vs->offsets.alloc(ob, &ix->pool);
        if (ob) SLG_HIP(hipMemcpy(vs->offsets.p, d.vec_offsets, ob, hipMemcpyHostToDevice));
        vs->values.alloc(vb, &ix->pool);
        if (vb) SLG_HIP(hipMemcpy(vs->values.p, d.vec_values, vb, hipMemcpyHostToDevice));
        vs->dim = d.vec_dim;
        vs->n_rows = d.vec_rows;
        vf->per_seg[s] = std::move(vs);
      }
      ns.vfields.push_back(std::move(vf));
      id = (int)ns.vfields.size();
    });
  });
  return rc == SLG_OK ? id : rc;
}

int slg_index_quantize_vector_field(slg_index *ix, uint32_t field) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    {
      const auto cur = ix->snapshot();
      SLG_REQUIRE(field <= cur->vfields.size(), "unknown vector field id");
      if (cur->vcopies.count(field)) return;  // (copies follow the index's updates: nothing to redo)
    }
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      SLG_REQUIRE(field <= cur.vfields.size(), "unknown vector field id");
      if (cur.vcopies.count(field)) return;
      const size_t n_segs = cur.segs.size();
      auto vc = std::make_shared<VecCopyField>();
      vc->per_seg.resize(n_segs);
      for (size_t s = 0; s < n_segs; s++) {
        if (field == 0) {
          const PostingStore &ps = *cur.segs[s]->store;
          if (ps.vec_dim)
            vc->per_seg[s] = vs_quantize_store(ix, ps.d_vec_values.as<float>(), ps.vec_rows, ps.vec_dim);
        } else {
          const VecFieldHost &vf = *cur.vfields[field - 1];
          if (s < vf.per_seg.size() && vf.per_seg[s]) {
            const VecSegStore &st = *vf.per_seg[s];
            vc->per_seg[s] = vs_quantize_store(ix, st.values.as<float>(), st.n_rows, st.dim);
          }
        }
      }
      ns.vcopies[field] = std::move(vc);
    });
  });
}

int slg_index_fetch_vector_copy(slg_index *ix, uint32_t field, uint32_t seg, uint16_t *out_u16, float *out_norm,
                                uint32_t rows_cap) {
  int rows = 0;
  const int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    const auto st = ix->snapshot();
    const auto it = st->vcopies.find(field);
    SLG_REQUIRE(it != st->vcopies.end(), "vector field " + std::to_string(field) + " has no bf16 copy");
    SLG_REQUIRE(seg < st->segs.size(), "no such segment");
    const VecCopyField &vc = *it->second;
    if (seg >= vc.per_seg.size() || !vc.per_seg[seg]) return;  // (no vectors of the field in this segment)
    const VecCopySeg &c = *vc.per_seg[seg];
    SLG_REQUIRE(c.n_rows <= 0x7FFFFFFFu, "more than 2^31 - 1 rows");
    rows = (int)c.n_rows;
    const uint32_t n = std::min(c.n_rows, rows_cap);
    if (n == 0) return;
    SLG_REQUIRE(out_u16 != nullptr && out_norm != nullptr, "output arrays are NULL");
    DeviceGuard g(ix->device);
    SLG_HIP(hipMemcpy2D(out_u16, (size_t)c.dim * 2, c.rows.p, (size_t)c.dim_pad * 2, (size_t)c.dim * 2, n,
                        hipMemcpyDeviceToHost));
    SLG_HIP(hipMemcpy(out_norm, c.norms.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  });
  return rc == SLG_OK ? rows : rc;
}

int slg_index_cluster_vector_field(slg_index *ix, uint32_t field, const slg_vector_lists_desc *per_segment,
                                   uint32_t n_segs) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      // every check before any device work
      SLG_REQUIRE(field <= cur.vfields.size(), "unknown vector field id");
      SLG_REQUIRE(n_segs == cur.segs.size(), "n_segs is not the index's segment count");
      SLG_REQUIRE(per_segment != nullptr || n_segs == 0, "per_segment is NULL");
      auto store_of = [&](size_t s, const uint32_t **offs, const float **vals, uint32_t *rows, uint32_t *dim,
                          int32_t *metric) { vec_store_of(cur, field, s, offs, vals, rows, dim, metric); };
      for (uint32_t s = 0; s < n_segs; s++) {
        const slg_vector_lists_desc &d = per_segment[s];
        if (d.n_lists == 0 || d.n_lists == SLG_KEEP_VECTOR_LISTS) continue;
        if (d.n_lists > SLG_MAX_VECTOR_LISTS) throw SlgError(SLG_ERR_UNSUPPORTED, "n_lists > SLG_MAX_VECTOR_LISTS");
        SLG_REQUIRE(d.centroids != nullptr, "centroids is NULL with n_lists > 0");
        const uint32_t *offs = nullptr;
        const float *vals = nullptr;
        uint32_t rows = 0, dim = 0;
        int32_t metric = 0;
        store_of(s, &offs, &vals, &rows, &dim, &metric);
        SLG_REQUIRE(dim != 0, "n_lists > 0 on segment " + std::to_string(s) + ", which has no vectors in the field");
      }
      auto vl = std::make_shared<VecListField>();
      const auto old = cur.vlists.find(field);
      vl->per_seg.resize(n_segs);
      for (uint32_t s = 0; s < n_segs; s++) {
        const slg_vector_lists_desc &d = per_segment[s];
        if (d.n_lists == SLG_KEEP_VECTOR_LISTS) {
          if (old != cur.vlists.end() && s < old->second->per_seg.size()) vl->per_seg[s] = old->second->per_seg[s];
          continue;
        }
        if (d.n_lists == 0) continue;
        const uint32_t *offs = nullptr;
        const float *vals = nullptr;
        uint32_t rows = 0, dim = 0;
        int32_t metric = 0;
        store_of(s, &offs, &vals, &rows, &dim, &metric);
        vl->per_seg[s] = vs_cluster_store(ix, offs, vals, cur.segs[s]->n_docs, rows, dim, metric, d.centroids, d.n_lists);
      }
      ns.vlists[field] = std::move(vl);
    });
  });
}

int slg_index_train_vector_field(slg_index *ix, uint32_t field, const slg_vector_train_desc *per_segment,
                                 uint32_t n_segs, slg_vector_train_stats *out_stats) {
  return guarded([&] {
    auto trained = [](const slg_vector_train_desc &d) { return d.n_lists != 0 && d.n_lists != SLG_KEEP_VECTOR_LISTS; };
    if (per_segment)  // the iters check comes first, before the index is looked at
      for (uint32_t s = 0; s < n_segs; s++)
        if (trained(per_segment[s]) && per_segment[s].iters > SLG_MAX_VECTOR_TRAIN_ITERS)
          throw SlgError(SLG_ERR_UNSUPPORTED, "iters > SLG_MAX_VECTOR_TRAIN_ITERS");
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    std::vector<slg_vector_train_stats> stats;  // (sized once n_segs is known to be the index's)
    update_state(ix, false, [&](const IndexState &cur, IndexState &ns) {
      // every check before any device work
      SLG_REQUIRE(field <= cur.vfields.size(), "unknown vector field id");
      SLG_REQUIRE(n_segs == cur.segs.size(), "n_segs is not the index's segment count");
      SLG_REQUIRE(per_segment != nullptr || n_segs == 0, "per_segment is NULL");
      stats.assign(n_segs, slg_vector_train_stats{0u, 0u, 0u, 0u});
      for (uint32_t s = 0; s < n_segs; s++) {
        const slg_vector_train_desc &d = per_segment[s];
        if (!trained(d)) continue;
        if (d.n_lists > SLG_MAX_VECTOR_LISTS) throw SlgError(SLG_ERR_UNSUPPORTED, "n_lists > SLG_MAX_VECTOR_LISTS");
        const uint32_t *offs = nullptr;
        const float *vals = nullptr;
        uint32_t rows = 0, dim = 0;
        int32_t metric = 0;
        vec_store_of(cur, field, s, &offs, &vals, &rows, &dim, &metric);
        SLG_REQUIRE(dim != 0, "n_lists > 0 on segment " + std::to_string(s) + ", which has no vectors in the field");
        SLG_REQUIRE(d.init != nullptr || d.n_lists <= rows,
                    "init is NULL and n_lists exceeds the " + std::to_string(rows) + " rows of segment " +
                        std::to_string(s) + "'s store");
      }
      auto vl = std::make_shared<VecListField>();
      const auto old = cur.vlists.find(field);
      vl->per_seg.resize(n_segs);
      for (uint32_t s = 0; s < n_segs; s++) {
        const slg_vector_train_desc &d = per_segment[s];
        if (d.n_lists == SLG_KEEP_VECTOR_LISTS) {
          if (old != cur.vlists.end() && s < old->second->per_seg.size()) vl->per_seg[s] = old->second->per_seg[s];
          continue;
        }
        if (d.n_lists == 0) continue;
        const uint32_t *offs = nullptr;
        const float *vals = nullptr;
        uint32_t rows = 0, dim = 0;
        int32_t metric = 0;
        vec_store_of(cur, field, s, &offs, &vals, &rows, &dim, &metric);
        vl->per_seg[s] = vs_train_store(ix, offs, vals, cur.segs[s]->n_docs, rows, dim, metric, d.init, d.n_lists,
                                        d.iters, &stats[s]);
      }
      ns.vlists[field] = std::move(vl);
    });
    if (out_stats)
      for (uint32_t s = 0; s < n_segs; s++) out_stats[s] = stats[s];
  });
}

int slg_index_fetch_vector_lists(slg_index *ix, uint32_t field, uint32_t seg, uint32_t *out_list_begin,
                                 uint32_t *out_docs, float *out_centroids, uint32_t lists_cap, uint32_t docs_cap) {
  int lists = 0;
  const int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    const auto st = ix->snapshot();
    SLG_REQUIRE(field <= st->vfields.size(), "unknown vector field id");
    SLG_REQUIRE(seg < st->segs.size(), "no such segment");
    const auto it = st->vlists.find(field);
    if (it == st->vlists.end()) return;  // (never clustered)
    const VecListField &vl = *it->second;
    if (seg >= vl.per_seg.size() || !vl.per_seg[seg]) return;  // (unclustered, or no vectors of the field)
    const VecListSeg &ls = *vl.per_seg[seg];
    lists = (int)ls.n_lists;
    DeviceGuard g(ix->device);
    const uint32_t nl = std::min(ls.n_lists, lists_cap), nd = std::min(ls.n_listed, docs_cap);
    if (nl) {
      SLG_REQUIRE(out_list_begin != nullptr && out_centroids != nullptr, "output arrays are NULL");
      SLG_HIP(hipMemcpy(out_list_begin, ls.list_begin.p, ((size_t)nl + 1) * 4, hipMemcpyDeviceToHost));
      SLG_HIP(hipMemcpy(out_centroids, ls.centroids.p, (size_t)nl * ls.dim * 4, hipMemcpyDeviceToHost));
    }
    if (nd) {
      SLG_REQUIRE(out_docs != nullptr, "out_docs is NULL");
      SLG_HIP(hipMemcpy(out_docs, ls.docs.p, (size_t)nd * 4, hipMemcpyDeviceToHost));
    }
  });
  return rc == SLG_OK ? lists : rc;
}

}  // extern "C"
