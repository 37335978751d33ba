// slg_explain.hpp — explain (slg_batch_explain): per returned row of a batch that has run, the first-pass score of
// its doc, the value of every score function that gave the doc one, and the end of the chain — the reference's
// HitExplanation (api/reader.rs:90-97; evaluate_compiled_score, :418-613).  The semantics in full:
// include/searchlite_gpu.h.
//
// The score stages rewrite the candidates' scores in place, so the base score of a row is gone when the batch has
// run: it is computed again from the posting lists.  The primitive is rescore_kernel's (slg_rescore.hpp): one
// workgroup of 256 threads per query, a lane owns up to four rows (row = thread + 256 * r) and runs their binary
// searches side by side; ceil(log2 df) dependent 4-byte loads narrow a list to one posting, one more compares it, one
// reads the impact.  A search stays inside [off, off + df).  What differs from the rescore:
//   * the lists are the batch's own TermRef rows, which exist per (query, segment) sub-query and hold only the terms
//     with postings there: a lane's four rows may lie in four segments, so each row walks its own row of terms (its
//     own count, its own leaf ends); the query's rows of all segments are staged in LDS, 20 bytes a term, and found
//     through the [nq x n_segs] table of sub-query indices the host built when it planned the batch;
//   * the arithmetic is the scoring kernels' for flat plans (slg_score_uni4.hpp, slg_score_multi.hpp), bit for bit: a
//     leaf's terms added in term order from +0.0, EVERY leaf of the sub-query closed into the root (one without a
//     posting of the doc adds its +0.0 and enters the maximum as 0.0), Sum from -0.0, DisMax max + tie * (sum - max)
//     with the maximum starting at max_init; plan 0 is the Sum whose every term is a leaf (0.0 + x == -0.0 + (0.0 + x)
//     for every x, so one form serves both);
//   * no sort and no WaveTopK: rows keep their place.
// The stages then run over that base in the batch's order, one row at a time, through the device functions the
// stage kernels themselves call (fscore_candidate, script_candidate) with the segment per lane instead of per wave:
// the query's records are still block-uniform scalar loads, the columns and bitmaps of a row's segment vector loads.
// A lane reads the base score of a row back from the output array it wrote it to itself, so the row loop needs no
// per-row registers and nothing goes to scratch (profiles/explain_resource_usage.txt).
//
// FULL = false compiles the kernel without ln / log1p / log2 / pow, as fscore_kernel's lean form.
#pragma once

#include "slg_fscore.hpp"
#define SLG_SCRIPT_DEVICE_FUNCTIONS_ONLY
#include "slg_script.hpp"

namespace slg {

constexpr int kExplainThreads = 256;
constexpr int kExplainRows = 4;  // rows per lane
constexpr uint32_t kExplainMaxRows = kExplainThreads * kExplainRows;
constexpr uint32_t kExplainMaxFuncs = kFscoreMaxFuncs + 1u;
constexpr uint32_t kExplainNoSq = 0xFFFFFFFFu;
constexpr uint32_t kExplainScript = 5u;  // = SLG_EXPLAIN_SCRIPT_SCORE (the function kinds: explain_type)
constexpr uint32_t kExStageFscore = 1u, kExStageScript = 2u, kExStageScriptFirst = 4u;

// the (query, segment) sub-query of a workgroup's query, as its lanes read it from LDS
struct ExplainSeg {
  uint32_t term_begin, n_terms;  // the sub-query's TermRef rows (n_terms 0: the pair has no sub-query)
  uint32_t begin, n_use;         // its first entry of the LDS table; its entries there (= n_terms: the host sized the table)
  uint32_t plan;
  float tie, max_init;
};

struct ExplainParams {
  const SegDev *segs;
  uint32_t n_segs;
  const RoundQuery *sq;
  const TermRef *terms;
  const uint32_t *q_seg_sq;  // [nq * n_segs] sub-query of the pair, or kExplainNoSq
  const uint32_t *row_doc, *row_seg;  // the batch's rows [nq * k]
  const float *row_score;
  const uint32_t *row_count;  // [nq]
  uint32_t nq, k, rows;
  uint32_t max_table;  // entries of the LDS table: >= the term rows of every query, >= 2
  uint32_t stages;     // kExStage*
  const FscoreQuery *fs_queries;
  const FscoreFn *fs_fns;
  const ColumnDev *fs_cols;
  const uint32_t *const *fs_filters;
  const ScriptQuery *sc_queries;
  const ScriptInstr *sc_instrs;
  const ColumnDev *sc_cols;
  const float *rs_rescore_score;  // a rescore batch: its side arrays [nq * k]; else null
  const uint32_t *rs_rescored;
  // the output, zeroed before the launch: [nq * rows], the entries [nq * rows * kExplainMaxFuncs]
  float *base_score, *final_score;
  uint32_t *n_functions, *fn_type;
  int32_t *fn_field;
  float *fn_value;
  uint32_t *rescored;
  float *rescore_score, *combined_score;
};

inline size_t explain_lds_bytes(uint32_t max_table, uint32_t n_segs) {
  return (size_t)max_table * 20 + (size_t)n_segs * sizeof(ExplainSeg);
}

// SLG_EXPLAIN_* of a function (FscoreFn::kinds)
__device__ __forceinline__ uint32_t explain_type(uint32_t kinds) {
  const uint32_t kind = kinds & 0xFFu;
  return kind == kFsDecay ? 2u + ((kinds >> 16) & 0xFFu) : kind;
}

template <bool FULL>
__global__ void __launch_bounds__(kExplainThreads) explain_kernel(ExplainParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int R = kExplainRows;
  uint64_t *s_off = reinterpret_cast<uint64_t *>(smem);  // [max_table]
  uint32_t *s_df = reinterpret_cast<uint32_t *>(s_off + p.max_table);
  float *s_w = reinterpret_cast<float *>(s_df + p.max_table);
  uint32_t *s_leaf = s_df + 2 * (size_t)p.max_table;
  ExplainSeg *s_seg = reinterpret_cast<ExplainSeg *>(s_leaf + p.max_table);  // [n_segs]
  const uint32_t tid = threadIdx.x;
  const uint32_t q = blockIdx.x, k = p.k, n_segs = p.n_segs, rows = p.rows;
  uint32_t n = p.row_count[q];
  n = n < k ? n : k;
  n = n < rows ? n : rows;
  n = n < kExplainMaxRows ? n : kExplainMaxRows;  // (the host refused more: a guard, not a path)
  if (n == 0u) return;
  const uint32_t *const rdoc = p.row_doc + (size_t)q * k;
  const uint32_t *const rseg = p.row_seg + (size_t)q * k;
  const size_t out0 = (size_t)q * rows;

  // ---- the query's sub-queries, then their term rows, into LDS ----
  for (uint32_t s = tid; s < n_segs; s += kExplainThreads) {
    ExplainSeg e{0u, 0u, 0u, 0u, 0u, 0.0f, 0.0f};
    const uint32_t sqi = p.q_seg_sq[(size_t)q * n_segs + s];
    if (sqi != kExplainNoSq) {
      const RoundQuery rq = p.sq[sqi];
      e.term_begin = rq.term_begin;
      e.n_terms = rq.n_terms;
      e.plan = rq.plan & 0xFFu;  // (bits 8..: min_match, which accepts docs and scores none)
      e.tie = rq.tie;
      e.max_init = rq.max_init;
    }
    s_seg[s] = e;
  }
  __syncthreads();
  for (uint32_t s = tid; s < n_segs; s += kExplainThreads) {
    uint32_t at = 0u;
    for (uint32_t j = 0; j < s; j++) at += s_seg[j].n_terms;
    at = at < p.max_table ? at : p.max_table;
    const uint32_t room = p.max_table - at, nt = s_seg[s].n_terms;
    s_seg[s].begin = at;  // (nobody reads begin and n_use before the barrier below)
    s_seg[s].n_use = nt < room ? nt : room;  // (the host sized the table for every query: a guard, not a path)
  }
  __syncthreads();
  for (uint32_t s = 0; s < n_segs; s++) {
    const ExplainSeg e = s_seg[s];
    for (uint32_t i = tid; i < e.n_use; i += kExplainThreads) {
      const TermRef t = p.terms[e.term_begin + i];
      s_off[e.begin + i] = t.off;
      s_df[e.begin + i] = t.df;
      s_w[e.begin + i] = t.weight;
      s_leaf[e.begin + i] = t.leaf;
    }
  }
  // this lane's rows
  typedef const __attribute__((address_space(1))) uint32_t *gdoc_t;
  typedef const __attribute__((address_space(1))) float *gimp_t;
  bool valid[R];
  uint32_t doc[R], seg[R];
  gdoc_t docs[R];
  gimp_t imps[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const uint32_t i = tid + kExplainThreads * r;
    valid[r] = i < n;
    doc[r] = valid[r] ? rdoc[i] : 0u;
    seg[r] = valid[r] ? rseg[i] : 0u;
    valid[r] = valid[r] && seg[r] < n_segs;  // (a row of no segment is looked up nowhere)
    seg[r] = valid[r] ? seg[r] : 0u;
    const SegDev sd = p.segs[seg[r]];
    docs[r] = (gdoc_t)sd.docs;
    imps[r] = (gimp_t)sd.imps;
  }
  __syncthreads();

  // ---- the first-pass score of every row: its segment's terms in term order, every leaf closed into the root ----
  uint32_t beg[R], nt[R], plan[R];
  float tie[R], mx[R], tot[R], la[R];
  uint32_t max_nt = 0u;
#pragma unroll
  for (int r = 0; r < R; r++) {
    const ExplainSeg e = s_seg[seg[r]];
    beg[r] = e.begin;
    nt[r] = valid[r] ? e.n_use : 0u;
    plan[r] = e.plan;
    tie[r] = e.tie;
    mx[r] = e.max_init;
    tot[r] = e.plan == 2u ? 0.0f : -0.0f;  // a DisMax sums from 0.0, a Sum from -0.0 (f32's Sum identity)
    la[r] = 0.0f;
    max_nt = nt[r] > max_nt ? nt[r] : max_nt;
  }
  for (uint32_t ti = 0; ti < max_nt; ti++) {
    uint64_t off[R];
    uint32_t cnt[R], pos[R];
    float wt[R];
    bool close[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const bool active = ti < nt[r];
      const uint32_t at = active ? beg[r] + ti : 0u;  // (entry 0 exists: max_table >= 2)
      const bool last = ti + 1u >= nt[r];
      const uint32_t next_leaf = s_leaf[last ? at : at + 1u];
      off[r] = s_off[at];
      cnt[r] = active ? s_df[at] : 0u;
      wt[r] = s_w[at];
      pos[r] = 0u;
      // plan 0: every term its own leaf; else a leaf ends where the next term's leaf differs (the rows are sorted by leaf)
      close[r] = active && (plan[r] == 0u || last || next_leaf != s_leaf[at]);
    }
    // the last posting <= doc of each row's list (or posting 0): every probe lies in [off, off + df)
    bool more = false;
#pragma unroll
    for (int r = 0; r < R; r++) more = more || cnt[r] > 1u;
    while (more) {
      uint32_t v[R], half[R];
#pragma unroll
      for (int r = 0; r < R; r++) {
        half[r] = cnt[r] >> 1;
        v[r] = 0u;
        if (cnt[r] > 1u) v[r] = docs[r][off[r] + pos[r] + half[r]];
      }
      more = false;
#pragma unroll
      for (int r = 0; r < R; r++) {
        if (cnt[r] > 1u) {
          pos[r] = v[r] <= doc[r] ? pos[r] + half[r] : pos[r];
          cnt[r] -= half[r];
        }
        more = more || cnt[r] > 1u;
      }
    }
    uint32_t hit_doc[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      hit_doc[r] = kDocEnd;
      if (cnt[r] != 0u) hit_doc[r] = docs[r][off[r] + pos[r]];
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
      const bool found = cnt[r] != 0u && hit_doc[r] == doc[r];
      float imp = 0.0f;
      if (found) imp = imps[r][off[r] + pos[r]];
      if (found) la[r] += imp * wt[r];  // score_tf: impact * weight, then the leaf's sum (no contraction)
      if (close[r]) {
        tot[r] += la[r];
        mx[r] = fmaxf(mx[r], la[r]);
        la[r] = 0.0f;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; r++) {
    const uint32_t i = tid + kExplainThreads * r;
    if (i < n) p.base_score[out0 + i] = plan[r] == 2u ? mx[r] + tie[r] * (tot[r] - mx[r]) : tot[r];
  }

  // ---- the stages over that base, one row at a time (a lane reads back what it stored itself) ----
  const bool has_fs = (p.stages & kExStageFscore) != 0u, has_sc = (p.stages & kExStageScript) != 0u;
  const bool script_first = (p.stages & kExStageScriptFirst) != 0u;
  FscoreQuery fq{};
  if (has_fs) fq = load_const(p.fs_queries + q);
  const bool fs_work = has_fs && rfl(fq.work) != 0u;
  const uint32_t n_fns = rfl(fq.n_fns), modes = rfl(fq.modes);
  const uint32_t score_mode = modes & 0xFFu, boost_mode = (modes >> 8) & 0xFFu, flags = (modes >> 16) & 0xFFu;
  const FscoreFn *const fn_row = p.fs_fns + rfl(fq.fn_begin);
  ScriptQuery scq{};
  if (has_sc) scq = load_const(p.sc_queries + q);
  const uint32_t n_instrs = rfl(scq.n_instrs), n_fields = rfl(scq.n_fields);
  const ScriptInstr *const prog = p.sc_instrs + rfl(scq.instr_begin);
  for (uint32_t i = tid; i < n; i += kExplainThreads) {
    const uint32_t d = rdoc[i];
    uint32_t sg = rseg[i];
    const bool live = sg < n_segs;
    sg = live ? sg : 0u;
    float score = p.base_score[out0 + i];
    const size_t e0 = (out0 + i) * kExplainMaxFuncs;
    uint32_t nf = 0u;
    if (n_instrs != 0u && script_first) {
      bool none;
      score = script_candidate<false>(scq, prog, n_instrs, n_fields, p.sc_cols, n_segs, sg, d, live, score, none);
      p.fn_type[e0 + nf] = kExplainScript;
      p.fn_field[e0 + nf] = -1;
      p.fn_value[e0 + nf] = score;
      nf++;
    }
    if (fs_work) {
      bool accept;
      score = fscore_candidate<FULL, false>(fq, fn_row, n_fns, score_mode, boost_mode, flags, p.fs_cols, p.fs_filters, n_segs,
                                            sg, d, live, score, accept, [&](uint32_t kinds, int32_t field, float val) {
                                              if (nf < kExplainMaxFuncs) {  // (at most kFscoreMaxFuncs + 1: a guard)
                                                p.fn_type[e0 + nf] = explain_type(kinds);
                                                p.fn_field[e0 + nf] = field;
                                                p.fn_value[e0 + nf] = val;
                                                nf++;
                                              }
                                            });
    }
    if (n_instrs != 0u && !script_first && nf < kExplainMaxFuncs) {
      bool none;
      score = script_candidate<false>(scq, prog, n_instrs, n_fields, p.sc_cols, n_segs, sg, d, live, score, none);
      p.fn_type[e0 + nf] = kExplainScript;
      p.fn_field[e0 + nf] = -1;
      p.fn_value[e0 + nf] = score;
      nf++;
    }
    p.n_functions[out0 + i] = nf;
    if (p.rs_rescored != nullptr) {  // a rescore batch (no stage): the row's own score and the batch's side arrays
      const size_t ri = (size_t)q * k + i;
      const uint32_t flag = p.rs_rescored[ri];
      score = p.row_score[ri];
      p.rescored[out0 + i] = flag;
      p.rescore_score[out0 + i] = p.rs_rescore_score[ri];
      p.combined_score[out0 + i] = flag != 0u ? score : 0.0f;
    }
    p.final_score[out0 + i] = score;
  }
}

}  // namespace slg
