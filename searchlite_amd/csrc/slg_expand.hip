// slg_expand.hip — slg_expand_batch: the requests checked and their ranges found on the host copies of the
// dictionaries, the scan's tables onto the device, its two kernels (slg_expand.hpp), the rows back, and the host
// merge (slg_expand_merge.cpp).  (slg_index_set_terms: slg_index.hip, beside the other per-segment stores.)
#include "slg_host.hpp"

#include <chrono>

#include "slg_expand.hpp"

using namespace slghost;

static_assert(slg::kExpandWave == SLG_EXPAND_WAVE && slg::kExpandThreads == SLG_EXPAND_WORKGROUP &&
                  slg::kExpandChunk == SLG_EXPAND_CHUNK && slg::kExpandMaxChars == SLG_MAX_EXPAND_CHARS,
              "the scan's geometry as the ABI states it");
static_assert(slg::kExpandFuzzy == SLG_EXPAND_FUZZY && slg::kExpandPrefix == SLG_EXPAND_PREFIX &&
                  slg::kExpandWildcard == SLG_EXPAND_WILDCARD, "the kinds");

namespace {
struct PhaseMs {
  double scan = 0.0, merge = 0.0;
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

int slg_expand_batch(slg_index *ix, const slg_expand_req *reqs, uint32_t n_reqs, uint32_t *out_offsets,
                     uint32_t key_capacity, uint32_t *out_term_ids, uint8_t *out_distance) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(reqs != nullptr || n_reqs == 0, "expand: reqs is NULL");
    SLG_REQUIRE(out_offsets != nullptr, "expand: out_offsets is NULL");
    SLG_REQUIRE((out_term_ids == nullptr) == (out_distance == nullptr),
                "expand: out_term_ids and out_distance are both NULL (a size query) or both given");
    phase_ms() = PhaseMs();
    std::vector<slgexpand::Request> rq;
    rq.reserve(n_reqs);
    for (uint32_t r = 0; r < n_reqs; r++) rq.push_back(slgexpand::check_request(reqs[r], r));
    const auto S = ix->snapshot();
    const uint32_t n_segs = (uint32_t)S->segs.size();
    std::vector<const slgexpand::Dict *> dicts(n_segs);
    for (uint32_t s = 0; s < n_segs; s++) {
      SLG_REQUIRE(s < S->terms.size() && S->terms[s], "expand: segment " + std::to_string(s) + " has no term dictionary (slg_index_set_terms)");
      dicts[s] = &S->terms[s]->dict;
    }

    // the scan's tables: a pair per (request, segment) with a non-empty range, its chunks, its rows
    const auto t_scan = std::chrono::steady_clock::now();
    std::vector<slg::ExpandReqDev> rdev(n_reqs);
    std::vector<slg::ExpandPairDev> pairs;
    std::vector<uint32_t> chunk_pair;
    std::vector<int64_t> pair_of((size_t)n_reqs * n_segs, -1);
    uint64_t total_rows = 0;
    for (uint32_t r = 0; r < n_reqs; r++) {
      slg::ExpandReqDev &d = rdev[r];
      d.kind = rq[r].kind;
      d.max_edits = rq[r].max_edits;
      d.n_chars = (uint32_t)rq[r].cps.size();
      d.field_bytes = (uint32_t)rq[r].field_key.size();
      d.field_chars = rq[r].field_chars;
      std::copy(rq[r].cps.begin(), rq[r].cps.end(), d.cp);
      if (!rq[r].scan) continue;
      for (uint32_t s = 0; s < n_segs; s++) {
        uint32_t lo, hi;
        slgexpand::prefix_range(*dicts[s], rq[r].range_key, lo, hi);
        if (lo == hi) continue;
        const uint32_t rows = (uint32_t)std::min<uint64_t>(slgexpand::rows_needed(rq[r], s), hi - lo);
        SLG_REQUIRE(total_rows + rows < (1ull << 31) && chunk_pair.size() < (1u << 24), "expand: the batch's ranges are too large for one call");
        pair_of[(size_t)r * n_segs + s] = (int64_t)pairs.size();
        pairs.push_back(slg::ExpandPairDev{r, s, lo, hi, rows, (uint32_t)total_rows, (uint32_t)chunk_pair.size(), 0u});
        chunk_pair.insert(chunk_pair.end(), (hi - lo + slg::kExpandChunk - 1) / slg::kExpandChunk, (uint32_t)(pairs.size() - 1));
        total_rows += rows;
      }
    }
    const size_t n_pairs = pairs.size(), n_chunks = chunk_pair.size(), n_slabs = n_chunks * slg::kExpandWaves;
    std::vector<uint32_t> row_pos(total_rows), pair_total(n_pairs);
    std::vector<uint8_t> row_dist(total_rows);
    if (n_chunks) {
      DeviceGuard g(ix->device);
      hipStream_t st;
      {
        std::lock_guard<std::mutex> lk(ix->mu);
        st = ix->stream;
      }
      Staging sg(&ix->pool, st);
      slg::ExpandParams p{};
      p.reqs = sg.up(rdev.data(), rdev.size());
      p.segs = S->d_term_segs.as<const slg::ExpandSegDev>();
      p.pairs = sg.up(pairs.data(), n_pairs);
      p.chunk_pair = sg.up(chunk_pair.data(), n_chunks);
      p.ballots = sg.up<uint64_t>(nullptr, n_slabs * slg::kExpandIters);
      p.slab_count = sg.up<uint32_t>(nullptr, n_slabs);
      p.row_pos = sg.up<uint32_t>(nullptr, total_rows);
      p.row_dist = sg.up<uint8_t>(nullptr, total_rows);
      p.pair_total = sg.up<uint32_t>(nullptr, n_pairs);
      hipLaunchKernelGGL(slg::expand_count_kernel, dim3((uint32_t)n_chunks), dim3(slg::kExpandThreads), 0, st, p);
      SLG_HIP(hipGetLastError());
      hipLaunchKernelGGL(slg::expand_emit_kernel, dim3((uint32_t)n_chunks), dim3(slg::kExpandThreads), 0, st, p);
      SLG_HIP(hipGetLastError());
      sg.down(row_pos.data(), p.row_pos, total_rows);
      sg.down(row_dist.data(), p.row_dist, total_rows);
      sg.down(pair_total.data(), p.pair_total, n_pairs);
      SLG_HIP(hipStreamSynchronize(st));
    }
    phase_ms().scan = ms_since(t_scan);

    // the reference's loop over the rows
    const auto t_merge = std::chrono::steady_clock::now();
    std::vector<uint32_t> ids;
    std::vector<uint8_t> dist;
    std::vector<slgexpand::Rows> rows(n_segs);
    for (uint32_t r = 0; r < n_reqs; r++) {
      out_offsets[r] = (uint32_t)dist.size();
      for (uint32_t s = 0; s < n_segs; s++) {
        rows[s] = slgexpand::Rows();
        const int64_t pi = pair_of[(size_t)r * n_segs + s];
        if (pi < 0) continue;
        const slg::ExpandPairDev &pr = pairs[(size_t)pi];
        rows[s] = slgexpand::Rows{row_pos.data() + pr.row_base, row_dist.data() + pr.row_base,
                                  std::min(pair_total[(size_t)pi], pr.rows)};
        for (uint32_t i = 0; i < rows[s].n; i++)  // (what the host goes on to index its copy with)
          if (rows[s].pos[i] < pr.lo || rows[s].pos[i] >= pr.hi)
            throw SlgError(SLG_ERR_INTERNAL, "expand: the scan returned a position outside its range");
      }
      slgexpand::merge_request(rq[r], dicts.data(), n_segs, rows.data(), ids, dist);
      SLG_REQUIRE(dist.size() < (1ull << 31), "expand: too many keys for one call");
    }
    out_offsets[n_reqs] = (uint32_t)dist.size();
    phase_ms().merge = ms_since(t_merge);
    if (!out_term_ids) return;
    SLG_REQUIRE(dist.size() <= key_capacity, "expand: key_capacity " + std::to_string(key_capacity) + " is too small for " +
                                                 std::to_string(dist.size()) + " keys");
    if (!dist.empty()) {
      std::memcpy(out_term_ids, ids.data(), ids.size() * 4);
      std::memcpy(out_distance, dist.data(), dist.size());
    }
  });
}

int slg_expand_phase_ms(slg_index *ix, double *scan_ms, double *merge_ms) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    if (scan_ms) *scan_ms = phase_ms().scan;
    if (merge_ms) *merge_ms = phase_ms().merge;
  });
}

}  // extern "C"
