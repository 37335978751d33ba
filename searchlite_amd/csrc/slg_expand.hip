// slg_expand.hip — slg_expand_batch: the requests checked and their ranges found on the host copies of the
// dictionaries, the scan's tables onto the device, its kernels (slg_expand.hpp; slg_expand_regex.hpp: the count
// kernel of regex requests, whose chunks are the tail of the chunk table), the rows back, and the host merge
// (slg_expand_merge.cpp).  (slg_index_set_terms: slg_index.hip, beside the other per-segment stores.)
#include "slg_host.hpp"

#include <atomic>
#include <chrono>
#include <exception>
#include <system_error>
#include <thread>

#include "slg_expand.hpp"
#include "slg_expand_regex.hpp"

using namespace slghost;

static_assert(slg::kExpandRegex == SLG_EXPAND_REGEX && slg::kRegexMaxStates == SLG_MAX_REGEX_STATES &&
                  slg::kRegexMaxTable == SLG_MAX_REGEX_TABLE, "the regex kind and its limits as the ABI states them");

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

// check_request for every request; the error of the lowest failing request, as a loop in order would report it.
// Checking a regex request compiles its pattern (tens of microseconds each), so a batch with many of them is dealt
// over a few threads; any other batch is checked in place
constexpr uint32_t kRegexCheckParallelFrom = 64, kRegexCheckThreads = 8;
void check_requests(const slg_expand_req *reqs, uint32_t n_reqs, std::vector<slgexpand::Request> &rq) {
  uint32_t n_regex = 0;
  for (uint32_t r = 0; r < n_reqs; r++) n_regex += reqs[r].kind == SLG_EXPAND_REGEX;
  if (n_regex < kRegexCheckParallelFrom) {
    for (uint32_t r = 0; r < n_reqs; r++) rq[r] = slgexpand::check_request(reqs[r], r);
    return;
  }
  std::vector<std::exception_ptr> failed(n_reqs);
  std::atomic<uint32_t> next{0};
  const auto work = [&] {
    for (uint32_t r = next.fetch_add(1); r < n_reqs; r = next.fetch_add(1)) {
      try {
        rq[r] = slgexpand::check_request(reqs[r], r);
      } catch (...) {
        failed[r] = std::current_exception();
      }
    }
  };
  std::vector<std::thread> pool;
  pool.reserve(kRegexCheckThreads);
  try {
    for (uint32_t t = 1; t < kRegexCheckThreads; t++) pool.emplace_back(work);
  } catch (const std::system_error &) {  // (fewer threads: the ones that run take the rest)
  }
  work();
  for (auto &th : pool) th.join();
  for (uint32_t r = 0; r < n_reqs; r++)
    if (failed[r]) std::rethrow_exception(failed[r]);
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
    std::vector<slgexpand::Request> rq(n_reqs);
    check_requests(reqs, n_reqs, rq);
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
    // regex requests: each one's DFA in one blob (slg_expand_regex.hpp), and their chunks behind all others, so
    // that they are one contiguous run of the chunk table: its own count kernel takes that run
    std::vector<slg::RegexReqDev> rxdev(n_reqs, slg::RegexReqDev{0u, 0u, 0u, 0u});
    std::vector<uint8_t> blobs;
    size_t n_plain_chunks = 0;
    for (uint64_t i = 0; i < 2ull * n_reqs; i++) {  // the requests twice: the other kinds, then regex
      const uint32_t r = (uint32_t)(i % n_reqs);
      if (i == n_reqs) n_plain_chunks = chunk_pair.size();
      const bool is_regex = rq[r].kind == SLG_EXPAND_REGEX;
      if (is_regex != (i >= n_reqs)) continue;
      slg::ExpandReqDev &d = rdev[r];
      d.kind = rq[r].kind;
      d.max_edits = rq[r].max_edits;
      d.n_chars = is_regex ? 0u : (uint32_t)rq[r].cps.size();  // (the device never reads a regex's code points)
      d.field_bytes = (uint32_t)rq[r].field_key.size();
      d.field_chars = rq[r].field_chars;
      if (!is_regex) std::copy(rq[r].cps.begin(), rq[r].cps.end(), d.cp);
      if (!rq[r].scan) continue;
      if (is_regex) {
        const slgregex::Dfa &f = rq[r].dfa;
        const size_t table = f.table.size();
        if (f.n_states < 2 || f.n_states > SLG_MAX_REGEX_STATES || table != (size_t)f.n_states * f.n_classes ||
            table > SLG_MAX_REGEX_TABLE || f.accept.size() != slg::kRegexAcceptBytes ||
            *std::max_element(f.table.begin(), f.table.end()) >= f.n_states ||
            *std::max_element(f.class_of, f.class_of + 256) >= f.n_classes)
          throw SlgError(SLG_ERR_INTERNAL, "expand: a compiled regex outside its limits");
        const uint32_t table_bytes = (uint32_t)((table + 3) / 4 * 4);
        rxdev[r] = slg::RegexReqDev{(uint32_t)blobs.size(), f.n_states, f.n_classes, table_bytes};
        blobs.insert(blobs.end(), f.class_of, f.class_of + 256);
        blobs.insert(blobs.end(), f.table.begin(), f.table.end());
        blobs.resize(blobs.size() + (table_bytes - table), 0);
        blobs.insert(blobs.end(), f.accept.begin(), f.accept.end());
        SLG_REQUIRE(blobs.size() < (1ull << 31), "expand: the batch's regex tables are too large for one call");
      }
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
      if (n_plain_chunks) {
        hipLaunchKernelGGL(slg::expand_count_kernel, dim3((uint32_t)n_plain_chunks), dim3(slg::kExpandThreads), 0, st, p);
        SLG_HIP(hipGetLastError());
      }
      if (n_chunks > n_plain_chunks) {
        slg::ExpandRegexParams q{};
        q.p = p;
        q.rx = sg.up(rxdev.data(), rxdev.size());
        q.blobs = sg.up(blobs.data(), blobs.size());
        q.chunk_base = (uint32_t)n_plain_chunks;
        hipLaunchKernelGGL(slg::expand_regex_count_kernel, dim3((uint32_t)(n_chunks - n_plain_chunks)),
                           dim3(slg::kExpandThreads), 0, st, q);
        SLG_HIP(hipGetLastError());
      }
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
