// slg_explain.hip — slg_batch_explain: the arguments checked on the host (slg_explain_host.hpp), then one staging
// path: the table of sub-query indices onto the device, the zeroed output block, explain_kernel behind the batch's
// last kernel on the batch's stream, the arrays back into the caller's.  A post-pass: the batch is left as it is.
#include "slg_host.hpp"

#include "slg_explain.hpp"
#include "slg_explain_host.hpp"

using namespace slghost;

static_assert(slg::kExplainMaxRows == SLG_MAX_EXPLAIN_ROWS && slg::kExplainMaxFuncs == SLG_MAX_EXPLAIN_FUNCS, "header limits");
static_assert(slg::kFsWeight == SLG_EXPLAIN_WEIGHT && slg::kFsFieldValue == SLG_EXPLAIN_FIELD_VALUE_FACTOR &&
                  slg::kFsDecay + slg::kFsDecayExp == SLG_EXPLAIN_DECAY_EXP && slg::kFsDecay + slg::kFsDecayGauss == SLG_EXPLAIN_DECAY_GAUSS &&
                  slg::kFsDecay + slg::kFsDecayLinear == SLG_EXPLAIN_DECAY_LINEAR && slg::kExplainScript == SLG_EXPLAIN_SCRIPT_SCORE,
              "header entry types (explain_type)");
static_assert(sizeof(slg::ExplainSeg) == 28 && sizeof(slg::TermRef) == 32, "the LDS table: 20 bytes a term, 28 a segment");

extern "C" int slg_batch_explain(slg_batch *b, uint32_t rows, const slg_explain_out *out) {
  return guarded([&] {
    slgexplain::BatchFacts f;
    f.null_batch = b == nullptr;
    if (b) {
      f.detached = b->idx == nullptr;
      f.launched = b->launched && (b->nq == 0 || (b->d_out_doc && b->d_out_seg && b->d_out_count));
      f.scan = b->scan;
      f.hybrid = b->hybrid;
      f.nested = b->nested;
      f.deep = b->deep;
      f.rescore = b->rescore;
      f.last_sharded = b->last_sharded;
      f.max_table = b->ex_max_table;
    }
    slgexplain::check(f, rows, out);
    if (b->nq == 0) return;
    const IndexState &S = *b->snap;
    const uint32_t nq = b->nq, n_segs = (uint32_t)S.segs.size();
    if (b->ex_q_seg_sq.size() != (size_t)nq * n_segs)
      throw SlgError(SLG_ERR_INTERNAL, "explain: the batch has no table of sub-query indices");
    DeviceGuard g(b->idx->device);
    const hipStream_t st = locked_stream(b);
    Staging sg(&b->idx->pool, st);
    const size_t n = (size_t)nq * rows, ne = n * slg::kExplainMaxFuncs;
    uint32_t *const blk = sg.up<uint32_t>(nullptr, 6 * n + 3 * ne);  // the output, one block, zeroed
    SLG_HIP(hipMemsetAsync(blk, 0, (6 * n + 3 * ne) * 4, st));
    slg::ExplainParams p{};
    p.segs = S.d_segs.as<slg::SegDev>();
    p.n_segs = n_segs;
    p.sq = b->d_sq;
    p.terms = b->d_terms;
    p.q_seg_sq = sg.up(b->ex_q_seg_sq.data(), b->ex_q_seg_sq.size());
    p.row_doc = b->d_out_doc;
    p.row_seg = b->d_out_seg;
    p.row_score = b->d_out_score;
    p.row_count = b->d_out_count;
    p.nq = nq;
    p.k = b->k;
    p.rows = rows;
    p.max_table = (std::max(b->ex_max_table, 2u) + 1u) & ~1u;  // even: the 4-byte arrays behind the offsets stay 8-byte aligned
    bool full = false;
    if (b->fscore && b->fscore_work != 0u) {
      p.stages |= slg::kExStageFscore;
      unsigned char *base = b->d_fscore_desc.as<unsigned char>();
      p.fs_queries = reinterpret_cast<const slg::FscoreQuery *>(base);
      base += (size_t)nq * sizeof(slg::FscoreQuery);
      p.fs_fns = reinterpret_cast<const slg::FscoreFn *>(base);
      base += (size_t)b->fscore_fns * sizeof(slg::FscoreFn);
      p.fs_cols = reinterpret_cast<const slg::ColumnDev *>(base);
      base += (size_t)b->fscore_cols * sizeof(slg::ColumnDev);
      p.fs_filters = reinterpret_cast<const uint32_t *const *>(base);
      full = b->fscore_full;
    }
    if (b->script && b->script_work != 0u) {
      p.stages |= slg::kExStageScript | (b->script_first ? slg::kExStageScriptFirst : 0u);
      unsigned char *base = b->d_script_desc.as<unsigned char>();
      p.sc_queries = reinterpret_cast<const slg::ScriptQuery *>(base);
      base += (size_t)nq * sizeof(slg::ScriptQuery);
      p.sc_instrs = reinterpret_cast<const slg::ScriptInstr *>(base);
      base += (size_t)b->script_instrs * sizeof(slg::ScriptInstr);
      p.sc_cols = reinterpret_cast<const slg::ColumnDev *>(base);
    }
    if (b->rescore) {
      const size_t nk = (size_t)nq * b->k;
      p.rs_rescore_score = b->d_rs_side.as<const float>() + nk;
      p.rs_rescored = b->d_rs_side.as<const uint32_t>() + 2 * nk;
    }
    p.base_score = reinterpret_cast<float *>(blk);
    p.final_score = reinterpret_cast<float *>(blk + n);
    p.n_functions = blk + 2 * n;
    p.rescored = blk + 3 * n;
    p.rescore_score = reinterpret_cast<float *>(blk + 4 * n);
    p.combined_score = reinterpret_cast<float *>(blk + 5 * n);
    p.fn_type = blk + 6 * n;
    p.fn_field = reinterpret_cast<int32_t *>(blk + 6 * n + ne);
    p.fn_value = reinterpret_cast<float *>(blk + 6 * n + 2 * ne);
    const size_t lds = slg::explain_lds_bytes(p.max_table, n_segs);
    if (full) launch_kernel_lds(slg::explain_kernel<true>, p, dim3(nq), slg::kExplainThreads, lds, st);
    else launch_kernel_lds(slg::explain_kernel<false>, p, dim3(nq), slg::kExplainThreads, lds, st);
    sg.down(out->base_score, p.base_score, n);
    sg.down(out->final_score, p.final_score, n);
    sg.down(out->n_functions, p.n_functions, n);
    sg.down(out->fn_type, p.fn_type, ne);
    sg.down(out->fn_field, p.fn_field, ne);
    sg.down(out->fn_value, p.fn_value, ne);
    if (b->rescore) {
      sg.down(out->rescored, p.rescored, n);
      sg.down(out->rescore_score, p.rescore_score, n);
      sg.down(out->combined_score, p.combined_score, n);
    }
    SLG_HIP(wait_stream(st));
  });
}
