// slg_suggest.hip — slg_suggest_batch: the requests checked and their ranges found on the host copies of the
// dictionaries (slg_suggest_host.cpp), the tables onto the device, the scan's two kernels and the merge kernel
// (slg_suggest.hpp) back to back on one stream, the winners back, and their texts copied out of the host copies.
#include "slg_host.hpp"

#include <chrono>

#include "slg_suggest_host.hpp"

using namespace slghost;

static_assert(slg::kSuggestMaxCandidates == SLG_MAX_SUGGEST_CANDIDATES && slg::kSuggestMinScan == SLG_SUGGEST_MIN_SCAN &&
                  slg::kSuggestMergeThreads == SLG_SUGGEST_MERGE_WORKGROUP, "the suggester's constants as the ABI states them");

namespace {
struct PhaseMs {
  double device = 0.0, copy = 0.0;
};
PhaseMs &phase_ms() {
  thread_local PhaseMs p;
  return p;
}
double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

extern "C" {

int slg_suggest_batch(slg_index *ix, const slg_suggest_req *reqs, uint32_t n_reqs, uint32_t *out_offsets,
                      uint32_t option_capacity, float *out_score, uint64_t *out_doc_freq, uint32_t *out_text_offsets,
                      uint32_t text_capacity, char *out_text) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(reqs != nullptr || n_reqs == 0, "suggest: reqs is NULL");
    SLG_REQUIRE(out_offsets != nullptr, "suggest: out_offsets is NULL");
    const int given = (out_score != nullptr) + (out_doc_freq != nullptr) + (out_text_offsets != nullptr) + (out_text != nullptr);
    SLG_REQUIRE(given == 0 || given == 4,
                "suggest: out_score, out_doc_freq, out_text_offsets and out_text are all NULL (a size query) or all given");
    phase_ms() = PhaseMs();
    std::vector<slgsuggest::Request> rq;
    rq.reserve(n_reqs);
    for (uint32_t r = 0; r < n_reqs; r++) rq.push_back(slgsuggest::check_request(reqs[r], r));
    const auto S = ix->snapshot();
    const uint32_t n_segs = (uint32_t)S->segs.size();
    for (uint32_t s = 0; s < n_segs; s++)
      SLG_REQUIRE(s < S->terms.size() && S->terms[s], "suggest: segment " + std::to_string(s) + " has no term dictionary (slg_index_set_terms)");

    // the tables: a pair per (request, segment) with a non-empty range, its chunks, its rows; a request's options
    const auto t_dev = std::chrono::steady_clock::now();
    std::vector<slg::SuggestReqDev> rdev(n_reqs);
    std::vector<slg::ExpandPairDev> pairs;
    std::vector<uint32_t> chunk_pair, req_pair(n_reqs + 1, 0u), opt_base(n_reqs + 1, 0u);
    uint64_t total_rows = 0;
    for (uint32_t r = 0; r < n_reqs; r++) {
      rdev[r] = slgsuggest::device_request(rq[r]);
      req_pair[r] = (uint32_t)pairs.size();
      opt_base[r + 1] = opt_base[r] + (rq[r].scan ? std::min(rq[r].size, rq[r].cap) : 0u);
      SLG_REQUIRE(opt_base[r + 1] < (1u << 31), "suggest: too many options for one call");
      if (!rq[r].scan) continue;
      for (uint32_t s = 0; s < n_segs; s++) {
        uint32_t lo, hi;
        slgexpand::prefix_range(S->terms[s]->dict, rq[r].range_key, lo, hi);
        if (!rq[r].fuzzy) hi = slgsuggest::clip_plain(S->terms[s]->nonzero, lo, hi, rq[r].cap);
        if (lo == hi) continue;
        const uint32_t rows = std::min(rq[r].cap, hi - lo);
        SLG_REQUIRE(total_rows + rows < (1ull << 31) && chunk_pair.size() < (1u << 24), "suggest: the batch's ranges are too large for one call");
        pairs.push_back(slg::ExpandPairDev{r, s, lo, hi, rows, (uint32_t)total_rows, (uint32_t)chunk_pair.size(), 0u});
        chunk_pair.insert(chunk_pair.end(), (hi - lo + slg::kExpandChunk - 1) / slg::kExpandChunk, (uint32_t)(pairs.size() - 1));
        total_rows += rows;
      }
    }
    req_pair[n_reqs] = (uint32_t)pairs.size();
    const size_t n_pairs = pairs.size(), n_chunks = chunk_pair.size(), n_slabs = n_chunks * slg::kExpandWaves;
    const size_t n_slots = opt_base[n_reqs];
    std::vector<uint32_t> opt_seg(n_slots), opt_pos(n_slots), n_opts(n_reqs, 0u);
    std::vector<float> opt_score(n_slots);
    std::vector<uint64_t> opt_df(n_slots);
    if (n_chunks) {
      DeviceGuard g(ix->device);
      hipStream_t st;
      {
        std::lock_guard<std::mutex> lk(ix->mu);
        st = ix->stream;
      }
      Staging sg(&ix->pool, st);
      slg::SuggestScanParams p{};
      p.reqs = sg.up(rdev.data(), rdev.size());
      p.segs = S->d_suggest_segs.as<const slg::SuggestSegDev>();
      p.pairs = sg.up(pairs.data(), n_pairs);
      p.chunk_pair = sg.up(chunk_pair.data(), n_chunks);
      p.ballots = sg.up<uint64_t>(nullptr, n_slabs * slg::kExpandIters);
      p.slab_count = sg.up<uint32_t>(nullptr, n_slabs);
      p.row_pos = sg.up<uint32_t>(nullptr, total_rows);
      p.row_dist = sg.up<uint8_t>(nullptr, total_rows);
      p.row_df = sg.up<uint32_t>(nullptr, total_rows);
      p.pair_total = sg.up<uint32_t>(nullptr, n_pairs);
      slg::SuggestMergeParams m{};
      m.reqs = p.reqs;
      m.segs = p.segs;
      m.pairs = p.pairs;
      m.req_pair = sg.up(req_pair.data(), req_pair.size());
      m.row_pos = p.row_pos;
      m.row_dist = p.row_dist;
      m.row_df = p.row_df;
      m.pair_total = p.pair_total;
      m.opt_base = sg.up(opt_base.data(), (size_t)n_reqs);
      m.opt_seg = sg.up<uint32_t>(nullptr, n_slots);
      m.opt_pos = sg.up<uint32_t>(nullptr, n_slots);
      m.opt_score = sg.up<float>(nullptr, n_slots);
      m.opt_df = sg.up<uint64_t>(nullptr, n_slots);
      m.n_opts = sg.up<uint32_t>(nullptr, (size_t)n_reqs);
      hipLaunchKernelGGL(slg::suggest_count_kernel, dim3((uint32_t)n_chunks), dim3(slg::kExpandThreads), 0, st, p);
      SLG_HIP(hipGetLastError());
      hipLaunchKernelGGL(slg::suggest_emit_kernel, dim3((uint32_t)n_chunks), dim3(slg::kExpandThreads), 0, st, p);
      SLG_HIP(hipGetLastError());
      hipLaunchKernelGGL(slg::suggest_merge_kernel, dim3(n_reqs), dim3(slg::kSuggestMergeThreads), 0, st, m);
      SLG_HIP(hipGetLastError());
      sg.down(opt_seg.data(), m.opt_seg, n_slots);
      sg.down(opt_pos.data(), m.opt_pos, n_slots);
      sg.down(opt_score.data(), m.opt_score, n_slots);
      sg.down(opt_df.data(), m.opt_df, n_slots);
      sg.down(n_opts.data(), m.n_opts, (size_t)n_reqs);
      SLG_HIP(hipStreamSynchronize(st));
    }
    phase_ms().device = ms_since(t_dev);

    // the winners' texts from the host copies
    const auto t_copy = std::chrono::steady_clock::now();
    uint64_t n_options = 0, text_bytes = 0;
    for (uint32_t r = 0; r < n_reqs; r++) {
      out_offsets[r] = (uint32_t)n_options;
      if (n_opts[r] > opt_base[r + 1] - opt_base[r]) throw SlgError(SLG_ERR_INTERNAL, "suggest: the merge returned more options than a request can have");
      for (uint32_t i = 0; i < n_opts[r]; i++) {
        const size_t o = opt_base[r] + i;
        if (opt_seg[o] >= n_segs || opt_pos[o] >= S->terms[opt_seg[o]]->dict.n())
          throw SlgError(SLG_ERR_INTERNAL, "suggest: the merge returned a key outside its dictionary");
        const std::string_view key = S->terms[opt_seg[o]]->dict.key(opt_pos[o]);
        if (key.size() < rq[r].field_key.size()) throw SlgError(SLG_ERR_INTERNAL, "suggest: the merge returned a key of another field");
        const std::string_view text = key.substr(rq[r].field_key.size());
        if (given) {
          SLG_REQUIRE(n_options < option_capacity, "suggest: option_capacity " + std::to_string(option_capacity) + " is too small");
          SLG_REQUIRE(text_bytes + text.size() <= text_capacity, "suggest: text_capacity " + std::to_string(text_capacity) + " is too small");
          out_score[n_options] = opt_score[o];
          out_doc_freq[n_options] = opt_df[o];
          out_text_offsets[n_options] = (uint32_t)text_bytes;
          if (!text.empty()) std::memcpy(out_text + text_bytes, text.data(), text.size());
        }
        n_options++;
        text_bytes += text.size();
        SLG_REQUIRE(text_bytes < (1ull << 32), "suggest: too many text bytes for one call");
      }
    }
    out_offsets[n_reqs] = (uint32_t)n_options;
    if (given) {
      SLG_REQUIRE(n_options <= option_capacity, "suggest: option_capacity " + std::to_string(option_capacity) + " is too small");  // (out_text_offsets holds one more)
      out_text_offsets[n_options] = (uint32_t)text_bytes;
    } else {
      out_offsets[n_reqs + 1] = (uint32_t)text_bytes;
    }
    phase_ms().copy = ms_since(t_copy);
  });
}

int slg_suggest_phase_ms(slg_index *ix, double *device_ms, double *copy_ms) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    if (device_ms) *device_ms = phase_ms().device;
    if (copy_ms) *copy_ms = phase_ms().copy;
  });
}

}  // extern "C"
