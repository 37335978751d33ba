// slg_api.hip — host side of the C ABI declared in include/searchlite_gpu.h.
//
// Mirrors, for the GPU-eligible request shape, what IndexReader::search_segment does
// before and after the scorer call (searchlite-core/src/api/reader.rs:2971-3000 build the
// ScoredTerm list; :3075-3099 call the scorer; :2776-2778 merge across segments), but for
// a whole batch of queries at once.  The product path has NO CPU fallback: every entry
// point either runs the HIP kernels or fails with an error code.
#include "../../include/searchlite_gpu.h"

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <map>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "slg_kernels.hpp"
#include "slg_plan.hpp"
#include "slg_rerank.hpp"
#include "slg_score.hpp"
#include "slg_score_uni4.hpp"
#include "slg_score_multi.hpp"
#include "slg_vsearch.hpp"

namespace {

thread_local std::string g_last_error;
thread_local int g_last_code = SLG_OK;

using slgplan::SlgError;  // {code, message}; also what the host planner throws

#define SLG_HIP(expr)                                                                     \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess) {                                                               \
      int _code = (_e == hipErrorOutOfMemory) ? SLG_ERR_OOM : SLG_ERR_DEVICE;             \
      throw SlgError(_code, std::string(#expr) + ": " + hipGetErrorString(_e));           \
    }                                                                                     \
  } while (0)

#define SLG_REQUIRE(cond, msg)                              \
  do {                                                      \
    if (!(cond)) throw SlgError(SLG_ERR_INVALID, (msg));    \
  } while (0)

template <typename F>
int guarded(F &&f) {
  try {
    g_last_error.clear();
    g_last_code = SLG_OK;
    f();
    return SLG_OK;
  } catch (const SlgError &e) {
    g_last_error = e.what();
    g_last_code = e.code;
  } catch (const std::bad_alloc &) {
    g_last_error = "host allocation failed";
    g_last_code = SLG_ERR_OOM;
  } catch (const std::exception &e) {
    g_last_error = e.what();
    g_last_code = SLG_ERR_INTERNAL;
  } catch (...) {
    g_last_error = "unknown error";
    g_last_code = SLG_ERR_INTERNAL;
  }
  return g_last_code;
}

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

// Freed batch buffers are kept for the next batch: hipMalloc / hipFree cost ~100 us each and
// hipFree synchronizes the device, which would serialize host threads that serve batches
// concurrently.  Size classes: powers of two from 4 KiB to 1 MiB, above that eight steps per
// octave (<= 12.5 % over-allocation).  The pool is bounded (slg_tuning.pool_cap_mb) and is the
// first thing given back when the device runs out of memory: every allocation of the library that
// fails with hipErrorOutOfMemory drains it and tries once more, so parked blocks of size classes
// nobody asks for any more can never starve a new batch, a second index or the application.
struct BufPool {
  std::mutex mu;
  std::multimap<size_t, void *> free_;
  size_t pooled = 0;
  // (config 4 on one GPU holds ~1 GB of work buffers per 8192-query batch and keeps three batches
  //  alive: with a 4 GB cap every batch ended in hipFree + hipMalloc, which synchronise the device)
  size_t cap = 24ull << 30;
  // pinned staging images of slg_batch_prepare* (descriptor uploads), owned by the index: taken
  // for one prepare call, handed back afterwards, released with the index (a thread_local image
  // would outlive its thread's usefulness and leak when caller threads come and go)
  std::vector<std::pair<void *, size_t>> images;
  static size_t size_class(size_t n) {  // powers of two up to 1 MiB, then eighths of an octave
    size_t c = 4096;
    while (c < n && c < (1u << 20)) c <<= 1;
    if (c >= n) return c;
    while ((c << 1) < n) c <<= 1;  // c <= n < 2c
    const size_t step = c >> 3;
    return c + ((n - c + step - 1) / step) * step;
  }
  // a free block of class cls, or the next larger one within 25 % (its size goes back in *got)
  void *get(size_t cls, size_t *got) {
    std::lock_guard<std::mutex> lk(mu);
    auto it = free_.lower_bound(cls);
    if (it == free_.end() || it->first > cls + cls / 4) return nullptr;
    void *p = it->second;
    *got = it->first;
    pooled -= it->first;
    free_.erase(it);
    return p;
  }
  bool put(void *p, size_t cls) {
    std::lock_guard<std::mutex> lk(mu);
    if (pooled + cls > cap) return false;
    free_.emplace(cls, p);
    pooled += cls;
    return true;
  }
  // give every parked block back to the runtime (largest first); returns the bytes freed
  size_t drain() {
    std::multimap<size_t, void *> take;
    {
      std::lock_guard<std::mutex> lk(mu);
      take.swap(free_);
      pooled = 0;
    }
    size_t freed = 0;
    for (auto it = take.rbegin(); it != take.rend(); ++it) {
      (void)hipFree(it->second);
      freed += it->first;
    }
    return freed;
  }
  // a pinned host image of at least n bytes (hipHostMallocPortable: usable from any device)
  void *take_image(size_t n, size_t *got) {
    {
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 0; i < images.size(); i++)
        if (images[i].second >= n) {
          void *p = images[i].first;
          *got = images[i].second;
          images[i] = images.back();
          images.pop_back();
          return p;
        }
      if (images.size() >= 16) {  // only too-small ones are parked: drop one
        (void)hipHostFree(images.back().first);
        images.pop_back();
      }
    }
    const size_t want = std::max<size_t>((n * 5) / 4, 1u << 20);
    void *p = nullptr;
    if (hipHostMalloc(&p, want, hipHostMallocPortable) != hipSuccess) return nullptr;
    *got = want;
    return p;
  }
  void give_image(void *p, size_t bytes) {
    std::lock_guard<std::mutex> lk(mu);
    images.emplace_back(p, bytes);
  }
  ~BufPool() {
    for (auto &kv : free_) (void)hipFree(kv.second);
    for (auto &im : images) (void)hipHostFree(im.first);
  }
};

// hipMalloc that drains `pool` (may be null) and tries once more when the device is out of memory
static void *device_alloc(size_t n, BufPool *pool) {
  void *p = nullptr;
  hipError_t e = hipMalloc(&p, n);
  if (e == hipErrorOutOfMemory && pool && pool->drain() > 0) {
    (void)hipGetLastError();
    e = hipMalloc(&p, n);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    throw SlgError(e == hipErrorOutOfMemory ? SLG_ERR_OOM : SLG_ERR_DEVICE,
                   std::string("hipMalloc(") + std::to_string(n) + "): " + hipGetErrorString(e));
  }
  return p;
}

struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  BufPool *pool = nullptr;  // set: bytes is a size class and the block goes back to the pool
  // relief: a pool to drain if the device is out of memory (the block itself is not pooled)
  void alloc(size_t n, BufPool *relief = nullptr) {
    release();
    if (n == 0) n = 16;
    p = device_alloc(n, relief);
    bytes = n;
  }
  void alloc_pooled(BufPool *pl, size_t n) {
    release();
    size_t cls = BufPool::size_class(n ? n : 16);
    p = pl->get(cls, &cls);
    if (!p) p = device_alloc(cls, pl);
    bytes = cls;
    pool = pl;
  }
  void release() {
    if (p && !(pool && pool->put(p, bytes))) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    pool = nullptr;
  }
  ~DevBuf() { release(); }
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes), pool(o.pool) {
    o.p = nullptr;
    o.bytes = 0;
    o.pool = nullptr;
  }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      bytes = o.bytes;
      pool = o.pool;
      o.p = nullptr;
      o.bytes = 0;
      o.pool = nullptr;
    }
    return *this;
  }
  template <typename T>
  T *as() const {
    return static_cast<T *>(p);
  }
};

// What a staged segment keeps for as long as any version of it lives: the posting arrays in the
// padded device layout, and (slg_tuning.updatable) everything stage_impacts_kernel needs to derive the
// impacts again when live_docs changes (slg_index_update_deleted).  Immutable after staging.
struct PostingStore {
  uint32_t n_docs = 0, n_terms = 0, n_fields = 0;
  uint64_t n_postings = 0;
  uint64_t null_idx = 0;               // SegDev::null_idx
  std::vector<uint64_t> term_offsets;  // as given (unpadded); device position = + kListPad * term
  std::vector<float> avgdl;            // [n_fields]
  float k1 = 0.0f, b = 0.0f;
  bool has_term_field = false;
  bool updatable = false;
  DevBuf d_docs;                                        // padded doc ids
  DevBuf d_offs, d_tfs, d_tfield, d_avgdl, d_lenptrs;   // updatable only (else freed after staging)
  std::vector<DevBuf> d_lens;                           // updatable only: per-field doc lengths
  // vectors (field 0)
  uint32_t vec_dim = 0, vec_rows = 0;
  int32_t vec_metric = 0;
  DevBuf d_vec_offsets, d_vec_values;
  size_t device_bytes() const {
    size_t n = d_docs.bytes + d_offs.bytes + d_tfs.bytes + d_tfield.bytes + d_avgdl.bytes + d_lenptrs.bytes +
               d_vec_offsets.bytes + d_vec_values.bytes;
    for (auto &l : d_lens) n += l.bytes;
    return n;
  }
};

// One VERSION of a staged segment: what depends on live_docs and the tombstones (impacts, champion
// bounds, the bitmap).  Versions of one segment share its PostingStore.
struct SegHost {
  std::shared_ptr<PostingStore> store;
  uint32_t n_docs = 0, n_terms = 0;
  uint64_t n_postings = 0;
  uint64_t null_idx = 0;
  float docs = 0.0f;         // live_docs this version's idf values were computed with
  std::vector<float> champ;  // host mirror of d_champ [V * kChampions] (query planning)
  DevBuf d_imps, d_deleted, d_champ;
  size_t device_bytes() const { return d_imps.bytes + d_deleted.bytes + d_champ.bytes; }
};

// a vector field beyond the one in the segment descriptors (slg_index_add_vector_field): per segment
// shared stores (null: the segment has no vectors in the field)
struct VecSegStore {
  DevBuf offsets, values;
  uint32_t dim = 0;
};
struct VecFieldHost {
  uint32_t dim = 0;
  int32_t metric = 0;
  std::vector<std::shared_ptr<VecSegStore>> per_seg;
  DevBuf d_vsegs;  // slg::VecSegDev[n_segs] of the state this object belongs to
};

// a registered doc filter: per segment a reject bitmap (deleted | ~filter); null = the filter predates
// the segment (slg_index_add_segment) and cannot be used until it is registered again
struct FilterData {
  std::vector<std::shared_ptr<DevBuf>> per_seg;
  bool complete() const {
    for (auto &b : per_seg)
      if (!b) return false;
    return true;
  }
};

// a registered sort field (slg_index_add_sort_field_*): per segment the u64 key of each order and the
// presence bitmap; null = the field predates the segment (slg_index_add_segment)
struct SortColumn {
  DevBuf key[2];  // SLG_ORDER_ASC, SLG_ORDER_DESC
  DevBuf present;
};
struct SortFieldData {
  int kind = 0;  // 1 i64, 2 f64 (a cursor's value is encoded by it)
  std::vector<std::shared_ptr<SortColumn>> per_seg;
};

// One immutable state of the index (see "index updates" in searchlite_gpu.h).  Batches hold the state
// they were prepared on; the index holds the current one.
struct IndexState {
  uint64_t generation = 0;
  int device = 0;
  std::vector<std::shared_ptr<SegHost>> segs;
  DevBuf d_segs;   // slg::SegDev[n_segs]
  DevBuf d_vsegs;  // slg::VecSegDev[n_segs]
  DevBuf d_doc_base;  // u32[n_segs + 1]: first flat doc of each segment (slg_vector_search_batch*)
  uint64_t total_docs = 0;
  std::vector<std::shared_ptr<VecFieldHost>> vfields;  // field id f >= 1 is vfields[f - 1]
  std::vector<std::shared_ptr<FilterData>> filters;    // slot = filter id; null = free
  std::vector<const uint32_t *> reject_host;           // flattened [filter * n_segs + seg] device pointers
  DevBuf d_reject_table;                               // the same table on the device
  std::map<int, std::shared_ptr<SortFieldData>> sort_fields;  // by id (ids are not reused)
  ~IndexState() {
    // kernels of already-destroyed batches, or rerank calls on the index stream, may still read the
    // tables: retiring a state is rare (one per update), so wait for the device once
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

}  // namespace

struct slg_index {
  // work buffers of finished batches.  Shared with the batches (a batch that outlives the index
  // still returns its buffers somewhere valid); declared first: destroyed last
  BufPool pool;
  slg_tuning tune{};
  std::vector<slg_batch *> live;  // batches prepared on this index and not yet destroyed (under mu)
  int device = 0;
  hipStream_t own_stream = nullptr;
  // descriptor uploads of slg_batch_prepare*: non-blocking streams picked by caller thread.  A plain
  // hipMemcpy runs on the legacy default stream and waits for whatever the application has queued
  // there (config 4: the previous batch's all-gather, shard merge and D2H) — planning would then
  // serialise with the GPU work it is supposed to overlap
  static constexpr int kUploadStreams = 8;
  hipStream_t upload_streams[kUploadStreams] = {};
  hipStream_t stream = nullptr;
  std::shared_ptr<const IndexState> state;  // the current state (under mu)
  std::atomic<uint64_t> generation{0};      // = state->generation, readable without the lock
  std::mutex mu;
  std::mutex update_mu;  // serialises slg_index_update_* / add_filter / add_vector_field (taken before mu)
  int next_sort_field = 0;  // (under update_mu) sort field ids are never handed out again
  // profiling of the scoring kernel
  bool profile = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
  size_t prof_used = 0;
  // set by a scoring wave that had to give up on a round (chunk-loop guard): checked at fetch
  DevBuf d_error_flag;
  // work space of slg_vector_search_batch* (under mu; used on `stream` only, so a call that grows it
  // frees the old block with hipFree, which waits for the device)
  DevBuf vs_scratch;
  std::shared_ptr<const IndexState> snapshot() {
    std::lock_guard<std::mutex> lk(mu);
    return state;
  }
};

struct slg_batch {
  slg_index *idx = nullptr;
  std::shared_ptr<const IndexState> snap;  // the index state the batch was prepared on
  uint32_t nq = 0, k = 0;
  int strategy = 0;
  uint32_t n_sq = 0, n_slices = 0, n_terms = 0, n_boundaries = 0, max_terms = 0;
  bool uniform = false;  // every sub-query fits the one-list-per-slot kernel
  bool plan_batch = false;  // some sub-query has a score plan (multi kernel only)
  bool nested = false;      // some sub-query has a two-level plan (groups of leaves)
  bool deep = false;        // some sub-query has a score tree of more than two levels
  const slg::PlanNode *d_nodes = nullptr;
  bool pruned = false;      // some sub-query has non-essential lists (MaxScore)
  bool multi = false;    // many-term form of it (slg_score_multi.hpp); else the packed kernel
  uint64_t n_postings = 0, n_postings_essential = 0, n_rounds = 0;
  std::vector<uint64_t> q_postings;  // per query (stats.postings_advanced)
  bool launched = false;             // slg_batch_run was called at least once
  bool own_stream_set = false;       // slg_batch_set_stream: run on `stream` instead of the index's
  hipStream_t stream = nullptr;
  DevBuf d_desc;                     // packed descriptors
  const slg::RoundQuery *d_sq = nullptr;
  const slg::TermRef *d_terms = nullptr;
  const uint32_t *d_slice_sq = nullptr;
  const uint32_t *d_slice_seg = nullptr;
  const uint32_t *d_slice_order = nullptr;
  const slg::QueryRef *d_queries = nullptr;
  const uint32_t *d_bnd_coarse = nullptr;
  DevBuf d_bounds, d_rdoc, d_slice_tk, d_slice_doc, d_q_scored, d_slice_desc;
  DevBuf d_q_filter;       // [nq] 0 = none, f + 1 (select_topk_kernel); empty when unfiltered
  bool cand_mode = false;  // uniform kernel, k > 256: candidates + select_topk_kernel
  DevBuf d_cand, d_slice_cbeg, d_slice_ccnt;
  // field-sorted batch (slg_batch_prepare_sorted): candidates of every matched doc + select_sorted_kernel
  bool sorted = false;
  uint32_t score_k = 0;  // k the scoring kernel runs with (a sorted batch: slgplan::planning_k)
  uint32_t n_sort_parts = 0, sort_score_parts = 0, sort_desc_parts = 0;
  DevBuf d_sort_cols;  // slg::SortColDev[kSortMaxParts * n_segs]
  DevBuf d_matched;    // u64[nq] accepted docs (sorted and cursor batches)
  // cursor batch (slg_batch_prepare_after): score order (!sorted: select_topk_kernel<true>) or a field sort
  // (select_sorted_kernel<true>)
  bool after = false;
  DevBuf d_cursor;  // u32[nq * slg::kCursorStride]: has_cursor, then the key words of the select kernel
  DevBuf d_seen;    // u32[nq] the cursor's key was seen
  DevBuf d_out;  // doc | seg | score | count, contiguous
  uint32_t *d_out_doc = nullptr, *d_out_seg = nullptr, *d_out_count = nullptr;
  float *d_out_score = nullptr;
  DevBuf d_stamps;  // SLG_STAMPS diagnostic builds
  DevBuf d_blk_skip;  // block skipping: postings of non-essential lists that were never loaded (u64)
  // index-sharded runs (slg_batch_run_sharded): the gathered result blocks of all ranks and the merged
  // top-k doc | seg | score | count
  DevBuf d_gather, d_merged;
  slg_shard_group *shard_group = nullptr;  // the group of the last sharded run (timing goes there)
  hipEvent_t ev_shard[4] = {nullptr, nullptr, nullptr, nullptr};  // start | local kernels done | gathered | merged
  bool shard_timed = false;
  uint64_t n_postings_nonessential = 0;  // postings of the pruning-classified (non-essential) lists
};

namespace {

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    SLG_HIP(hipGetDevice(&prev));
    if (prev != dev) SLG_HIP(hipSetDevice(dev));
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

int kregs_for(uint32_t k) {
  if (k <= 64) return 1;
  if (k <= 128) return 2;
  if (k <= 256) return 4;
  if (k <= 512) return 8;
  return 16;
}

}  // namespace
namespace slg {
// defined in slg_score_inst.hip, one translation unit per KREGS
template <int KREGS>
void launch_score_kregs(const RoundScoreParams &sp, int kind, hipStream_t st);
template <> void launch_score_kregs<1>(const RoundScoreParams &, int, hipStream_t);
template <> void launch_score_kregs<2>(const RoundScoreParams &, int, hipStream_t);
template <> void launch_score_kregs<4>(const RoundScoreParams &, int, hipStream_t);
template <> void launch_score_kregs<8>(const RoundScoreParams &, int, hipStream_t);
template <> void launch_score_kregs<16>(const RoundScoreParams &, int, hipStream_t);
}  // namespace slg
namespace {

// kind: 2 many-term kernel (slg_score_multi.hpp), 3 many-term kernel with pruning-classified lists,
// 6 / 7 the few-term kernel (slg_score_uni4.hpp), <= 4 / 5..8 lists; 8 / 9: the same with score plans
// (flat Sum / DisMax over leaves)
int uniform_kind(uint32_t max_terms, bool plans) {
  const bool few = max_terms <= (uint32_t)slg::kUniMaxLists;
  if (plans) return few ? 8 : 9;
  return few ? 6 : 7;
}
void launch_score(const slg::RoundScoreParams &sp, int kind, hipStream_t st) {
#ifdef SLG_STAMPS  // diagnostic build: only the k <= 64 variant is compiled
  if (kregs_for(sp.k) != 1) throw SlgError(SLG_ERR_UNSUPPORTED, "stamps build supports k <= 64 only");
  slg::launch_score_kregs<1>(sp, kind, st);
  SLG_HIP(hipGetLastError());
  return;
#else
  switch (kregs_for(sp.k)) {
    case 1: slg::launch_score_kregs<1>(sp, kind, st); break;
    case 2: slg::launch_score_kregs<2>(sp, kind, st); break;
    case 4: slg::launch_score_kregs<4>(sp, kind, st); break;
    case 8: slg::launch_score_kregs<8>(sp, kind, st); break;
    default: slg::launch_score_kregs<16>(sp, kind, st); break;
  }
  SLG_HIP(hipGetLastError());
#endif
}

template <int KREGS>
void launch_merge_t(const slg::MergeParams &mp, hipStream_t st) {
  const uint32_t blocks = (mp.nq + slg::kWavesPerBlock - 1) / slg::kWavesPerBlock;
  hipLaunchKernelGGL((slg::merge_topk_kernel<KREGS>), dim3(blocks), dim3(256), 0, st, mp);
}
void launch_merge(const slg::MergeParams &mp, hipStream_t st) {
  switch (kregs_for(mp.k)) {
    case 1: launch_merge_t<1>(mp, st); break;
    case 2: launch_merge_t<2>(mp, st); break;
    case 4: launch_merge_t<4>(mp, st); break;
    case 8: launch_merge_t<8>(mp, st); break;
    default: launch_merge_t<16>(mp, st); break;
  }
  SLG_HIP(hipGetLastError());
}

template <int KREGS>
void launch_shard_merge_t(const slg::ShardMergeParams &mp, hipStream_t st) {
  const uint32_t blocks = (mp.nq + slg::kWavesPerBlock - 1) / slg::kWavesPerBlock;
  hipLaunchKernelGGL((slg::merge_shards_kernel<KREGS>), dim3(blocks), dim3(256), 0, st, mp);
}
void launch_shard_merge(const slg::ShardMergeParams &mp, hipStream_t st) {
  if (mp.k > 1024u) {  // beyond the register top-k: rank every entry by binary searches
    hipLaunchKernelGGL(slg::merge_shards_large_kernel, dim3(mp.nq), dim3(256), 0, st, mp);
    SLG_HIP(hipGetLastError());
    return;
  }
  switch (kregs_for(mp.k)) {
    case 1: launch_shard_merge_t<1>(mp, st); break;
    case 2: launch_shard_merge_t<2>(mp, st); break;
    case 4: launch_shard_merge_t<4>(mp, st); break;
    case 8: launch_shard_merge_t<8>(mp, st); break;
    default: launch_shard_merge_t<16>(mp, st); break;
  }
  SLG_HIP(hipGetLastError());
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

// Waiting for a stream is the blocking hipStreamSynchronize.  (Polling hipStreamQuery first — to spare a
// small batch the sleep / wake-up of the blocking wait — was built and measured: with 8 caller threads
// polling, config 2's host-inclusive rate fell from 11M to 2.2M queries/s and fetch + destroy grew from
// 0.28 to 1.36 ms per batch: the query takes a runtime lock the other threads' launches and copies need.)
static inline hipError_t wait_stream(hipStream_t st) { return hipStreamSynchronize(st); }

static inline hipStream_t batch_stream(const slg_batch *b) {
  return b->own_stream_set ? b->stream : b->idx->stream;
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
  for (auto &vf : cur.vfields) {  // the per-state table d_vsegs is rebuilt: own object, shared stores
    auto c = std::make_shared<VecFieldHost>();
    c->dim = vf->dim;
    c->metric = vf->metric;
    c->per_seg = vf->per_seg;
    n->vfields.push_back(std::move(c));
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

size_t state_device_bytes(const IndexState &s) {
  size_t n = s.d_segs.bytes + s.d_vsegs.bytes + s.d_reject_table.bytes + s.d_doc_base.bytes;
  for (auto &sh : s.segs) n += sh->device_bytes() + sh->store->device_bytes();
  for (auto &f : s.filters)
    if (f)
      for (auto &b : f->per_seg)
        if (b) n += b->bytes;
  for (auto &sf : s.sort_fields)
    for (auto &c : sf.second->per_seg)
      if (c) n += c->key[0].bytes + c->key[1].bytes + c->present.bytes;
  for (auto &vf : s.vfields) {
    n += vf->d_vsegs.bytes;
    for (auto &v : vf->per_seg)
      if (v) n += v->offsets.bytes + v->values.bytes;
  }
  return n;
}

}  // namespace

extern "C" {

uint32_t slg_abi_version(void) { return SLG_ABI_VERSION; }

const char *slg_last_error(void) { return g_last_error.c_str(); }
int slg_last_error_code(void) { return g_last_code; }

int slg_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    g_last_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e);
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
    const std::string keep = g_last_error;
    if (ix) slg_index_destroy(ix);
    g_last_error = keep;
    g_last_code = rc;
    return nullptr;
  }
  return ix;
}

namespace {
// free everything a batch holds on the device; with `to_pool` false the blocks go straight back
// to the runtime (the index and its pool are going away)
void release_batch_buffers(slg_batch *b, bool to_pool) {
  DevBuf *bufs[] = {&b->d_desc, &b->d_bounds, &b->d_rdoc, &b->d_slice_desc, &b->d_slice_tk, &b->d_slice_doc,
                    &b->d_q_scored, &b->d_q_filter, &b->d_cand, &b->d_slice_cbeg, &b->d_slice_ccnt,
                    &b->d_out, &b->d_stamps, &b->d_blk_skip, &b->d_gather, &b->d_merged};
  for (DevBuf *d : bufs) {
    if (!to_pool) d->pool = nullptr;
    d->release();
  }
}
}  // namespace

void slg_index_destroy(slg_index *ix) {
  if (!ix) return;
  int prev = -1;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(ix->device);
  (void)hipDeviceSynchronize();  // batches may run on streams of their own
  {
    // batches that outlive the index are detached: buffers freed, handle stays valid for
    // slg_batch_destroy, every other call on it fails with SLG_ERR_INVALID
    std::lock_guard<std::mutex> lk(ix->mu);
    for (slg_batch *b : ix->live) {
      release_batch_buffers(b, false);
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
  if (prev >= 0) (void)hipSetDevice(prev);
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
    std::lock_guard<std::mutex> ulk(ix->update_mu);
    const auto cur = ix->snapshot();
    DeviceGuard g(ix->device);
    hipStream_t st = ix->stream;
    const size_t n_segs = cur->segs.size();
    auto fd = std::make_shared<FilterData>();
    fd->per_seg.resize(n_segs);
    std::vector<DevBuf> tmp(n_segs);  // uploaded pass bitmaps / columns (freed on return)
    std::vector<DevBuf> marked(n_segs);  // docs that hold one of the terms (slg_index_add_filter_terms)
    SLG_REQUIRE(n_terms == 0 || term_ids != nullptr, "term_ids is NULL");
    for (size_t s = 0; s < n_segs; s++) {
      const SegHost &sh = *cur->segs[s];
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
    // the next state: the filter takes the lowest free id (ids of removed filters are reused, so the
    // pointer table stays as small as the number of filters alive at once).  Batches prepared on
    // earlier states keep their own table: nobody waits for the device here
    auto ns = copy_state(*cur);
    ns->generation = cur->generation;  // (filters do not change what a manifest snapshot sees)
    size_t slot = 0;
    while (slot < ns->filters.size() && ns->filters[slot]) slot++;
    if (slot == ns->filters.size()) ns->filters.emplace_back();
    ns->filters[slot] = std::move(fd);
    finish_state(ix, *ns);
    publish(ix, std::move(ns));
    id = (int)slot;
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
    std::lock_guard<std::mutex> ulk(ix->update_mu);
    const auto cur = ix->snapshot();
    DeviceGuard g(ix->device);
    SLG_REQUIRE(filter_id >= 0 && (size_t)filter_id < cur->filters.size() && cur->filters[filter_id],
                "unknown filter id");
    // batches prepared with the filter hold the state that owns its bitmaps and its table row: they
    // may still run.  The slot is free for the next add
    auto ns = copy_state(*cur);
    ns->generation = cur->generation;
    ns->filters[filter_id].reset();
    while (!ns->filters.empty() && !ns->filters.back()) ns->filters.pop_back();
    finish_state(ix, *ns);
    publish(ix, std::move(ns));
  });
}

// ---- sort fields (query/sort.rs:300-345) ---------------------------------------------------
namespace {
int add_sort_field_impl(slg_index *ix, int kind, const uint32_t *const *seg_offsets, const void *const *seg_values) {
  int id = -1;
  const int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(seg_offsets != nullptr, "seg_offsets is NULL");
    std::lock_guard<std::mutex> ulk(ix->update_mu);
    const auto cur = ix->snapshot();
    DeviceGuard g(ix->device);
    const size_t n_segs = cur->segs.size();
    auto fd = std::make_shared<SortFieldData>();
    fd->kind = kind;
    fd->per_seg.resize(n_segs);
    for (size_t s = 0; s < n_segs; s++) {
      const uint32_t n_docs = cur->segs[s]->n_docs;
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
    auto ns = copy_state(*cur);
    ns->generation = cur->generation;  // (as filters: a manifest snapshot sees no change)
    id = ix->next_sort_field++;
    ns->sort_fields[id] = std::move(fd);
    finish_state(ix, *ns);
    publish(ix, std::move(ns));
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
    std::lock_guard<std::mutex> ulk(ix->update_mu);
    const auto cur = ix->snapshot();
    DeviceGuard g(ix->device);
    SLG_REQUIRE(cur->sort_fields.count(sort_field_id) == 1, "unknown sort field id");
    auto ns = copy_state(*cur);
    ns->generation = cur->generation;
    ns->sort_fields.erase(sort_field_id);
    finish_state(ix, *ns);
    publish(ix, std::move(ns));
  });
}

// ---- index updates (api/writer.rs:106-240) ---------------------------------------------------
int slg_index_update_deleted(slg_index *ix, uint32_t seg, const uint8_t *deleted, float live_docs) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    std::lock_guard<std::mutex> ulk(ix->update_mu);
    const auto cur = ix->snapshot();
    SLG_REQUIRE(seg < cur->segs.size(), "no such segment");
    SLG_REQUIRE(live_docs >= 0.0f && live_docs <= (float)cur->segs[seg]->n_docs, "live_docs outside [0, n_docs]");
    const std::shared_ptr<PostingStore> &ps = cur->segs[seg]->store;
    if (!ps->updatable)
      throw SlgError(SLG_ERR_UNSUPPORTED, "index was created with slg_tuning.updatable = 0");
    DeviceGuard g(ix->device);
    auto sh = std::make_shared<SegHost>();
    derive_version(ix, ps, *sh, deleted, live_docs, StageTemps{});
    auto ns = copy_state(*cur);
    ns->segs[seg] = sh;
    // registered filters: reject = deleted | ~filter, so this segment's bitmaps take the new tombstones
    const size_t words = std::max<size_t>(((size_t)ps->n_docs + 31) / 32, 1);
    for (auto &f : ns->filters) {
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
    finish_state(ix, *ns);
    publish(ix, std::move(ns));
  });
}

int slg_index_add_segment(slg_index *ix, const slg_segment_desc *seg) {
  int ord = -1;
  const int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr && seg != nullptr, "index or segment descriptor is NULL");
    validate_segment(*seg, 0, ix->tune.validate != 0);
    std::lock_guard<std::mutex> ulk(ix->update_mu);
    const auto cur = ix->snapshot();
    DeviceGuard g(ix->device);
    auto sh = stage_segment(ix, *seg);
    auto ns = copy_state(*cur);
    ns->segs.push_back(std::move(sh));
    for (auto &f : ns->filters)  // no bitmap for the new segment: unusable until registered again
      if (f) {
        auto nf = std::make_shared<FilterData>(*f);
        nf->per_seg.resize(ns->segs.size());
        f = std::move(nf);
      }
    for (auto &sf : ns->sort_fields) {  // sort fields too: no column for the new segment
      auto nf = std::make_shared<SortFieldData>(*sf.second);
      nf->per_seg.resize(ns->segs.size());
      sf.second = std::move(nf);
    }
    for (auto &vf : ns->vfields) vf->per_seg.resize(ns->segs.size());
    finish_state(ix, *ns);
    ord = (int)ns->segs.size() - 1;
    publish(ix, std::move(ns));
  });
  return rc == SLG_OK ? ord : rc;
}

int slg_index_remove_segment(slg_index *ix, uint32_t seg) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    std::lock_guard<std::mutex> ulk(ix->update_mu);
    const auto cur = ix->snapshot();
    SLG_REQUIRE(seg < cur->segs.size(), "no such segment");
    SLG_REQUIRE(cur->segs.size() > 1, "the last segment of an index cannot be removed (add the replacement first)");
    DeviceGuard g(ix->device);
    auto ns = copy_state(*cur);
    ns->segs.erase(ns->segs.begin() + seg);
    for (auto &f : ns->filters)
      if (f) {
        auto nf = std::make_shared<FilterData>(*f);
        if (seg < nf->per_seg.size()) nf->per_seg.erase(nf->per_seg.begin() + seg);
        f = std::move(nf);
      }
    for (auto &sf : ns->sort_fields) {
      auto nf = std::make_shared<SortFieldData>(*sf.second);
      if (seg < nf->per_seg.size()) nf->per_seg.erase(nf->per_seg.begin() + seg);
      sf.second = std::move(nf);
    }
    for (auto &vf : ns->vfields)
      if (seg < vf->per_seg.size()) vf->per_seg.erase(vf->per_seg.begin() + seg);
    finish_state(ix, *ns);
    publish(ix, std::move(ns));
  });
}

int slg_index_device(const slg_index *ix) {
  if (!ix) {
    g_last_error = "index is NULL";
    g_last_code = SLG_ERR_INVALID;
    return SLG_ERR_INVALID;
  }
  return ix->device;
}

uint64_t slg_index_generation(const slg_index *ix) {
  return ix ? ix->generation.load(std::memory_order_acquire) : 0;  // (no lock: callers poll it per request)
}

slg_batch *slg_batch_prepare(slg_index *ix, uint32_t nq, const uint32_t *q_offsets,
                             const uint32_t *q_term_ids, const float *q_weights, uint32_t k,
                             int strategy) {
  return slg_batch_prepare_filtered(ix, nq, q_offsets, q_term_ids, q_weights, nullptr, k, strategy);
}

slg_batch *slg_batch_prepare_filtered(slg_index *ix, uint32_t nq, const uint32_t *q_offsets,
                                      const uint32_t *q_term_ids, const float *q_weights,
                                      const int32_t *q_filter, uint32_t k, int strategy) {
  return slg_batch_prepare_plan(ix, nq, q_offsets, q_term_ids, q_weights, nullptr, nullptr, nullptr,
                                nullptr, q_filter, k, strategy);
}

slg_batch *slg_batch_prepare_plan(slg_index *ix, uint32_t nq, const uint32_t *q_offsets,
                                  const uint32_t *q_term_ids, const float *q_weights,
                                  const uint32_t *q_leaf, const int32_t *q_plan, const float *q_tie,
                                  const uint32_t *q_nleaves, const int32_t *q_filter, uint32_t k,
                                  int strategy) {
  slg_score_plans pl{};
  pl.q_leaf = q_leaf;
  pl.q_plan = q_plan;
  pl.q_tie = q_tie;
  pl.q_nleaves = q_nleaves;
  return slg_batch_prepare_plans(ix, nq, q_offsets, q_term_ids, q_weights, &pl, q_filter, k, strategy);
}

}  // extern "C"

namespace {
// slg_batch_prepare_plans, (sort != nullptr) slg_batch_prepare_sorted, and (after) slg_batch_prepare_after
slg_batch *prepare_impl(slg_index *ix, uint32_t nq, const uint32_t *q_offsets, const uint32_t *q_term_ids,
                        const float *q_weights, const slg_score_plans *plans, const int32_t *q_filter,
                        const slg_sort_spec *sort, uint32_t k, int strategy, bool after = false,
                        const slg_sort_cursor *q_cursor = nullptr) {
  slg_batch *b = nullptr;
  int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(!after || q_cursor != nullptr, "q_cursor is NULL");
    if (sort) {  // (checked before planning: the planner never sees a sort spec it cannot run)
      if (sort->n_parts > SLG_MAX_SORT_PARTS)
        throw SlgError(SLG_ERR_UNSUPPORTED, "more than SLG_MAX_SORT_PARTS sort parts");
      SLG_REQUIRE(sort->n_parts >= 1, "a sort spec needs at least one part");
      for (uint32_t i = 0; i < sort->n_parts; i++)
        SLG_REQUIRE(sort->order[i] == SLG_ORDER_ASC || sort->order[i] == SLG_ORDER_DESC, "unknown sort order");
    }
    // Planning (slg_plan.cpp: a pure host function) reads only the immutable state the batch binds
    // to, so host threads may prepare batches for one index concurrently, also while an update builds
    // the next state; the index mutex is held just to take the snapshot.
    const std::shared_ptr<const IndexState> snap = ix->snapshot();
    std::vector<char> filter_live(snap->filters.size());
    for (size_t f = 0; f < snap->filters.size(); f++)
      filter_live[f] = snap->filters[f] && snap->filters[f]->complete() &&
                       snap->filters[f]->per_seg.size() == snap->segs.size();
    std::vector<slgplan::SegView> views(snap->segs.size());
    for (size_t s = 0; s < snap->segs.size(); s++) {
      const SegHost &sh = *snap->segs[s];
      views[s].n_docs = sh.n_docs;
      views[s].n_terms = sh.n_terms;
      views[s].term_offsets = sh.store->term_offsets.data();
      views[s].champ = sh.champ.empty() ? nullptr : sh.champ.data();
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
    in.filter_live = filter_live.data();
    in.n_filters = filter_live.size();
    in.sorted = sort != nullptr || after;
    // the columns of the sort parts in the batch's state: every part names a field with a column for every
    // segment (a field registered before slg_index_add_segment has none for the new one)
    std::vector<slg::SortColDev> sort_cols;
    uint32_t score_parts = 0, desc_parts = 0;
    if (sort) {
      const size_t n_segs = snap->segs.size();
      sort_cols.assign(slg::kSortMaxParts * std::max<size_t>(n_segs, 1), slg::SortColDev{nullptr, nullptr});
      for (uint32_t i = 0; i < sort->n_parts; i++) {
        if (sort->order[i] == SLG_ORDER_DESC) desc_parts |= 1u << i;
        if (sort->field[i] == SLG_SORT_SCORE) {
          score_parts |= 1u << i;
          continue;
        }
        const auto it = snap->sort_fields.find(sort->field[i]);
        SLG_REQUIRE(it != snap->sort_fields.end(), "unknown sort field id in part " + std::to_string(i));
        const SortFieldData &fd = *it->second;
        for (size_t s = 0; s < n_segs; s++) {
          SLG_REQUIRE(s < fd.per_seg.size() && fd.per_seg[s],
                      "sort field " + std::to_string(sort->field[i]) + " has no column for segment " + std::to_string(s) +
                          " (added after the field was registered)");
          const SortColumn &c = *fd.per_seg[s];
          sort_cols[i * n_segs + s] = slg::SortColDev{c.key[sort->order[i]].as<const unsigned long long>(),
                                                      c.present.as<const uint32_t>()};
        }
      }
    }
    // the cursors as the key words the select kernel compares (against the same snapshot's field kinds)
    std::vector<uint32_t> cursor_words;
    if (after) {
      int kind[SLG_MAX_SORT_PARTS] = {0, 0, 0, 0};
      const uint32_t n_parts = sort ? sort->n_parts : 0u;
      for (uint32_t i = 0; i < n_parts; i++)
        kind[i] = sort->field[i] == SLG_SORT_SCORE ? 0 : snap->sort_fields.at(sort->field[i])->kind;
      cursor_words.assign((size_t)std::max<uint32_t>(nq, 1) * slg::kCursorStride, 0u);
      for (uint32_t q = 0; q < nq; q++) {
        if (!q_cursor[q].has_cursor) continue;
        uint32_t *w = &cursor_words[(size_t)q * slg::kCursorStride];
        w[0] = 1u;
        try {
          slgplan::cursor_key(n_parts, kind, sort ? sort->order : nullptr, q_cursor[q], w + 1);
        } catch (const slgplan::SlgError &e) {
          throw SlgError(e.code, "query " + std::to_string(q) + ": " + e.what());
        }
      }
    }
    slgplan::Plan plan;
    slgplan::plan_batch(views, ix->tune, in, plan);

    DeviceGuard g(ix->device);
    b = new slg_batch();
    b->idx = ix;
    b->snap = snap;
    b->nq = nq;
    b->k = k;
    b->strategy = strategy;
    b->q_postings.swap(plan.q_postings);
    b->n_postings = plan.n_postings;
    b->n_postings_essential = plan.n_postings_essential;
    b->n_postings_nonessential = plan.n_postings_nonessential;
    b->n_rounds = plan.n_rounds;
    b->max_terms = plan.max_terms;
    b->uniform = plan.uniform;
    b->multi = plan.multi;
    b->plan_batch = plan.plan_batch;
    b->nested = plan.nested;
    b->deep = plan.deep;
    b->pruned = plan.pruned;
    b->cand_mode = plan.cand_mode;
    b->sorted = sort != nullptr;
    b->after = after;
    b->score_k = slgplan::planning_k(in);
    b->n_sq = (uint32_t)plan.sqs.size();
    b->n_terms = (uint32_t)plan.terms.size();
    b->n_slices = (uint32_t)plan.slice_sq.size();
    b->n_boundaries = (uint32_t)plan.n_bnd;

    // ---- the descriptor image: one H2D copy the caller waits for, outside any lock, on an upload
    // stream of its own.  (Measured against an image copied asynchronously on the batch's stream in
    // front of the kernels: that variant served 5.2-7.4M queries/s from 4-8 caller threads where
    // this one serves 8.0-8.8M — the stream-ordered copy delays each batch's first kernel.)  The
    // staging image is pinned, so the copy is one DMA at PCIe speed (26 MB: 0.6 ms; from pageable
    // memory 1-6 ms), and comes from the index's free list (a fresh 26 MB vector per config-4
    // batch spent half of its 5 ms in page faults); it goes back when prepare returns.
    const size_t total = plan.image_bytes;
    struct ImageLease {
      BufPool *pool;
      void *p = nullptr;
      size_t bytes = 0;
      ~ImageLease() {
        if (p) pool->give_image(p, bytes);
      }
    } lease{&ix->pool};
    lease.p = ix->pool.take_image(total ? total : 16, &lease.bytes);
    if (!lease.p) throw SlgError(SLG_ERR_OOM, "pinned staging image: hipHostMalloc failed");
    plan.pack(static_cast<unsigned char *>(lease.p));
    b->d_desc.alloc_pooled(&ix->pool, total);
    {
      hipStream_t us = ix->upload_streams[std::hash<std::thread::id>()(std::this_thread::get_id()) %
                                          slg_index::kUploadStreams];
      SLG_HIP(hipMemcpyAsync(b->d_desc.p, lease.p, total, hipMemcpyHostToDevice, us));
      SLG_HIP(wait_stream(us));
    }
    unsigned char *db = b->d_desc.as<unsigned char>();
    b->d_sq = reinterpret_cast<const slg::RoundQuery *>(db + plan.o_sq);
    b->d_terms = reinterpret_cast<const slg::TermRef *>(db + plan.o_terms);
    b->d_slice_sq = reinterpret_cast<const uint32_t *>(db + plan.o_slice);
    b->d_slice_seg = reinterpret_cast<const uint32_t *>(db + plan.o_sseg);
    b->d_slice_order = reinterpret_cast<const uint32_t *>(db + plan.o_sord);
    b->d_queries = reinterpret_cast<const slg::QueryRef *>(db + plan.o_q);
    b->d_bnd_coarse = reinterpret_cast<const uint32_t *>(db + plan.o_bc);
    b->d_nodes = reinterpret_cast<const slg::PlanNode *>(db + plan.o_nodes);
    b->d_bounds.alloc_pooled(&ix->pool, (size_t)plan.n_bounds * 4);
    b->d_rdoc.alloc_pooled(&ix->pool, (size_t)plan.n_bnd * 4);
    b->d_slice_desc.alloc_pooled(&ix->pool, (size_t)b->n_slices * sizeof(slg::SliceDesc));
    if (b->cand_mode) {
      b->d_cand.alloc_pooled(&ix->pool, (size_t)(plan.cand_total + 1) * 8);
      b->d_slice_cbeg.alloc_pooled(&ix->pool, (size_t)b->n_slices * 8);
      b->d_slice_ccnt.alloc_pooled(&ix->pool, (size_t)b->n_slices * 4);
    } else {
      b->d_slice_tk.alloc_pooled(&ix->pool, (size_t)b->n_slices * k * 4);
      b->d_slice_doc.alloc_pooled(&ix->pool, (size_t)b->n_slices * k * 4);
    }
    b->d_q_scored.alloc_pooled(&ix->pool, (size_t)nq * 4);
    // (from the pool like every per-batch buffer: a raw hipMalloc / hipFree per batch synchronises
    // the device and cost config 4's two-in-flight pipeline 60 %)
    if (b->pruned && !b->uniform && ix->tune.block_max) b->d_blk_skip.alloc_pooled(&ix->pool, ((size_t)nq + 1) * 8);
    if (!plan.q_filter.empty()) {
      b->d_q_filter.alloc_pooled(&ix->pool, (size_t)nq * 4);
      SLG_HIP(hipMemcpy(b->d_q_filter.p, plan.q_filter.data(), (size_t)nq * 4, hipMemcpyHostToDevice));
    }
    if (b->sorted) {
      b->n_sort_parts = sort->n_parts;
      b->sort_score_parts = score_parts;
      b->sort_desc_parts = desc_parts;
      b->d_sort_cols.alloc_pooled(&ix->pool, sort_cols.size() * sizeof(slg::SortColDev));
      SLG_HIP(hipMemcpy(b->d_sort_cols.p, sort_cols.data(), sort_cols.size() * sizeof(slg::SortColDev),
                        hipMemcpyHostToDevice));
    }
    if (b->sorted || b->after) b->d_matched.alloc_pooled(&ix->pool, (size_t)std::max<uint32_t>(nq, 1) * 8);
    if (b->after) {
      b->d_cursor.alloc_pooled(&ix->pool, cursor_words.size() * 4);
      SLG_HIP(hipMemcpy(b->d_cursor.p, cursor_words.data(), cursor_words.size() * 4, hipMemcpyHostToDevice));
      b->d_seen.alloc_pooled(&ix->pool, (size_t)std::max<uint32_t>(nq, 1) * 4);
    }
    b->d_out.alloc_pooled(&ix->pool, ((size_t)nq * k * 3 + nq + 1) * 4);  // (+ the error word: MergeParams::out_flag)
    b->d_out_doc = b->d_out.as<uint32_t>();
    b->d_out_seg = b->d_out_doc + (size_t)nq * k;
    b->d_out_score = reinterpret_cast<float *>(b->d_out_seg + (size_t)nq * k);
    b->d_out_count = b->d_out_seg + (size_t)nq * k * 2;
    {
      std::lock_guard<std::mutex> lk(ix->mu);
      ix->live.push_back(b);
    }
  });
  if (rc != SLG_OK) {
    const std::string keep = g_last_error;
    const int keep_code = g_last_code;
    delete b;
    g_last_error = keep;
    g_last_code = keep_code;
    return nullptr;
  }
  return b;
}
}  // namespace

extern "C" {

slg_batch *slg_batch_prepare_plans(slg_index *ix, uint32_t nq, const uint32_t *q_offsets,
                                   const uint32_t *q_term_ids, const float *q_weights,
                                   const slg_score_plans *plans, const int32_t *q_filter, uint32_t k,
                                   int strategy) {
  return prepare_impl(ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, nullptr, k, strategy);
}

slg_batch *slg_batch_prepare_sorted(slg_index *ix, uint32_t nq, const uint32_t *q_offsets,
                                    const uint32_t *q_term_ids, const float *q_weights,
                                    const slg_score_plans *plans, const int32_t *q_filter,
                                    const slg_sort_spec *sort, uint32_t k, int strategy) {
  if (!sort) {
    (void)guarded([&] { SLG_REQUIRE(false, "sort spec is NULL"); });
    return nullptr;
  }
  return prepare_impl(ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, sort, k, strategy);
}

slg_batch *slg_batch_prepare_after(slg_index *ix, uint32_t nq, const uint32_t *q_offsets,
                                   const uint32_t *q_term_ids, const float *q_weights,
                                   const slg_score_plans *plans, const int32_t *q_filter, const slg_sort_spec *sort,
                                   const slg_sort_cursor *q_cursor, uint32_t k, int strategy) {
  return prepare_impl(ix, nq, q_offsets, q_term_ids, q_weights, plans, q_filter, sort, k, strategy, true, q_cursor);
}

#define SLG_REQUIRE_LIVE(b) \
  SLG_REQUIRE((b) != nullptr && (b)->idx != nullptr, "batch is NULL or its index was destroyed")

int slg_batch_run(slg_batch *b) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    slg_index *ix = b->idx;
    const IndexState &S = *b->snap;  // the state the batch was prepared on (not the index's current one)
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard g(ix->device);
    hipStream_t st = batch_stream(b);
    b->launched = true;
    if (b->nq == 0) return;
    if (b->n_slices == 0) SLG_HIP(hipMemsetAsync(b->d_q_scored.p, 0, (size_t)b->nq * 4, st));
    if (b->n_slices > 0) {
      slg::RoundPartParams pp{};
      pp.sq = b->d_sq;
      pp.terms = b->d_terms;
      pp.n_sq = b->n_sq;
      pp.bnd_coarse = b->d_bnd_coarse;
      pp.segs = S.d_segs.as<slg::SegDev>();
      pp.bounds = b->d_bounds.as<uint32_t>();
      pp.rdoc = b->d_rdoc.as<uint32_t>();
      pp.q_scored = b->d_q_scored.as<uint32_t>();
      const bool skipping = b->d_blk_skip.p != nullptr;
      pp.skip_counts = skipping ? b->d_blk_skip.as<unsigned long long>() : nullptr;
      pp.slice_sq = b->d_slice_sq;
      pp.slice_order = b->d_slice_order;
      pp.slice_desc = b->d_slice_desc.as<slg::SliceDesc>();
      pp.nq = b->nq;
      // the blocked few-term kernel can cut its slices itself (slg_tuning.inline_cuts)
      const bool inline_cuts = b->uniform && (ix->tune.inline_cuts >= 0 ? ix->tune.inline_cuts != 0 : true);
      pp.n_boundaries = inline_cuts ? 0u : b->n_boundaries;
      pp.n_slices = b->n_slices;
      pp.tpb_shift = b->max_terms <= 4 ? 2u : 3u;
      const int score_kind =
          b->uniform ? uniform_kind(b->max_terms, b->plan_batch) : (b->pruned ? 3 : 2);
      const uint64_t pthreads = std::max<uint64_t>(
          std::max<uint64_t>((uint64_t)pp.n_boundaries << pp.tpb_shift, (uint64_t)b->nq + 1), b->n_slices);
      hipLaunchKernelGGL(slg::partition_rounds_kernel, dim3((uint32_t)((pthreads + 255) / 256)),
                         dim3(256), 0, st, pp);
      SLG_HIP(hipGetLastError());

      slg::RoundScoreParams sp{};
      sp.sq = b->d_sq;
      sp.terms = b->d_terms;
      sp.slice_sq = b->d_slice_sq;
      sp.slice_order = b->d_slice_order;
      sp.slice_desc = b->d_slice_desc.as<slg::SliceDesc>();
      sp.reject_table = S.d_reject_table.as<const uint32_t *>();
      sp.n_segs = (uint32_t)S.segs.size();
      sp.plan_batch = b->plan_batch ? (b->deep ? 4u : (b->nested ? 2u : 1u)) : 0u;
      sp.plan_nodes = b->d_nodes;
      sp.cand = b->d_cand.as<uint2>();
      sp.slice_cbeg = b->d_slice_cbeg.as<uint64_t>();
      sp.slice_ccnt = b->d_slice_ccnt.as<uint32_t>();
      sp.segs = S.d_segs.as<slg::SegDev>();
      sp.bounds = inline_cuts ? nullptr : b->d_bounds.as<uint32_t>();
      sp.rdoc = inline_cuts ? nullptr : b->d_rdoc.as<uint32_t>();
      sp.slice_tk = b->d_slice_tk.as<int32_t>();
      sp.slice_doc = b->d_slice_doc.as<uint32_t>();
      sp.q_scored = b->d_q_scored.as<uint32_t>();
      sp.n_slices = b->n_slices;
      sp.k = b->score_k;
      sp.block_skip = skipping ? 1u : 0u;
      sp.skip_counts = pp.skip_counts;
      sp.stamps = nullptr;
      sp.error_flag = ix->d_error_flag.as<uint32_t>();
#ifdef SLG_STAMPS
      b->d_stamps.alloc((size_t)b->n_slices * 96);
      sp.stamps = b->d_stamps.as<unsigned long long>();
#endif
      std::pair<hipEvent_t, hipEvent_t> *ev = nullptr;
      if (ix->profile) {
        if (ix->prof_used == ix->prof_events.size()) {
          hipEvent_t a, c;
          SLG_HIP(hipEventCreate(&a));
          SLG_HIP(hipEventCreate(&c));
          ix->prof_events.emplace_back(a, c);
        }
        ev = &ix->prof_events[ix->prof_used++];
        SLG_HIP(hipEventRecord(ev->first, st));
      }
      launch_score(sp, score_kind, st);
      if (ev) SLG_HIP(hipEventRecord(ev->second, st));
    }
    if (b->sorted) {  // (also without slices: every row is empty, every matched count 0)
      slg::SortedSelectParams sp{};
      sp.queries = b->d_queries;
      sp.slice_seg = b->d_slice_seg;
      sp.slice_cbeg = b->d_slice_cbeg.as<uint64_t>();
      sp.slice_ccnt = b->d_slice_ccnt.as<uint32_t>();
      sp.cand = b->d_cand.as<uint2>();
      sp.segs = S.d_segs.as<slg::SegDev>();
      sp.q_filter = b->d_q_filter.as<uint32_t>();
      sp.reject_table = S.d_reject_table.as<const uint32_t *>();
      sp.cols = b->d_sort_cols.as<const slg::SortColDev>();
      sp.n_segs = (uint32_t)S.segs.size();
      sp.n_parts = b->n_sort_parts;
      sp.score_parts = b->sort_score_parts;
      sp.desc_parts = b->sort_desc_parts;
      sp.out_doc = b->d_out_doc;
      sp.out_seg = b->d_out_seg;
      sp.out_score = b->d_out_score;
      sp.out_count = b->d_out_count;
      sp.out_matched = b->d_matched.as<unsigned long long>();
      sp.nq = b->nq;
      sp.k = b->k;
      sp.error_flag = ix->d_error_flag.as<uint32_t>();
      sp.out_flag = b->d_out_count + b->nq;
      if (b->after) {
        sp.cursor = b->d_cursor.as<const uint32_t>();
        sp.out_seen = b->d_seen.as<uint32_t>();
        hipLaunchKernelGGL(slg::select_sorted_kernel<true>, dim3(b->nq), dim3(slg::kSortedThreads), 0, st, sp);
      } else {
        hipLaunchKernelGGL(slg::select_sorted_kernel<false>, dim3(b->nq), dim3(slg::kSortedThreads), 0, st, sp);
      }
      SLG_HIP(hipGetLastError());
    } else if (b->after || (b->k > 0 && b->cand_mode && b->n_slices > 0)) {
      // (a cursor batch in score order runs the select also without slices or with k = 0: it writes the
      //  matched counts and seen flags)
      slg::SelectParams sp{};
      sp.queries = b->d_queries;
      sp.slice_seg = b->d_slice_seg;
      sp.slice_cbeg = b->d_slice_cbeg.as<uint64_t>();
      sp.slice_ccnt = b->d_slice_ccnt.as<uint32_t>();
      sp.cand = b->d_cand.as<uint2>();
      sp.segs = S.d_segs.as<slg::SegDev>();
      sp.q_filter = b->d_q_filter.as<uint32_t>();
      sp.reject_table = S.d_reject_table.as<const uint32_t *>();
      sp.n_segs = (uint32_t)S.segs.size();
      sp.out_doc = b->d_out_doc;
      sp.out_seg = b->d_out_seg;
      sp.out_score = b->d_out_score;
      sp.out_count = b->d_out_count;
      sp.nq = b->nq;
      sp.k = b->k;
      sp.error_flag = ix->d_error_flag.as<uint32_t>();
      sp.out_flag = b->d_out_count + b->nq;
      if (b->after) {
        sp.cursor = b->d_cursor.as<const uint32_t>();
        sp.out_matched = b->d_matched.as<unsigned long long>();
        sp.out_seen = b->d_seen.as<uint32_t>();
        hipLaunchKernelGGL(slg::select_topk_kernel<true>, dim3(b->nq), dim3(slg::kSelectThreads), 0, st, sp);
      } else {
        hipLaunchKernelGGL(slg::select_topk_kernel<false>, dim3(b->nq), dim3(slg::kSelectThreads), 0, st, sp);
      }
      SLG_HIP(hipGetLastError());
    } else if (b->k > 0) {
      slg::MergeParams mp{};
      mp.queries = b->d_queries;
      mp.slice_seg = b->d_slice_seg;
      mp.slice_tk = b->d_slice_tk.as<int32_t>();
      mp.slice_doc = b->d_slice_doc.as<uint32_t>();
      mp.out_doc = b->d_out_doc;
      mp.out_seg = b->d_out_seg;
      mp.out_score = b->d_out_score;
      mp.out_count = b->d_out_count;
      mp.nq = b->nq;
      mp.k = b->k;
      mp.error_flag = ix->d_error_flag.as<uint32_t>();
      mp.out_flag = b->d_out_count + b->nq;
      launch_merge(mp, st);
    } else {
      SLG_HIP(hipMemsetAsync(b->d_out_count, 0, ((size_t)b->nq + 1) * 4, st));  // (k = 0: nothing was scored)
    }
  });
}

int slg_batch_sync(slg_batch *b) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    DeviceGuard g(b->idx->device);
    SLG_HIP(hipStreamSynchronize(batch_stream(b)));
  });
}

// result blocks up to this size are fetched into pageable memory (see slg_batch_fetch)
static constexpr size_t kPageableFetchBytes = 256u << 10;

int slg_batch_fetch(slg_batch *b, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                    uint32_t *out_count, slg_stats *stats) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->nq == 0 || (out_count != nullptr), "out_count is NULL");
    SLG_REQUIRE(b->nq == 0 || b->k == 0 || (out_doc && out_seg && out_score), "output array is NULL");
    slg_index *ix = b->idx;
    DeviceGuard g(ix->device);
    hipStream_t st;
    {  // (not held while waiting: other host threads keep launching their batches)
      std::lock_guard<std::mutex> lk(ix->mu);
      st = batch_stream(b);
    }
    const size_t n = (size_t)b->nq * b->k;
    std::vector<uint32_t> scored;
    std::vector<unsigned long long> skipped;
    if (b->nq) {
      // the results are one contiguous block doc | seg | score | count | error word: ONE D2H copy.
      // Large blocks (config 4: 10 MB) go into a PINNED staging image of the index's pool: a pageable
      // destination makes the runtime stage the copy itself, chunk by chunk behind a lock that every
      // caller thread's copies share.  Small ones (config 2: 46 KB) are copied straight into a pageable
      // image: for them the runtime's own path is the faster one (measured on one box, 8 caller threads,
      // 20-step regions: 12.1-12.5M against 10.4-11.0M queries/s with the pinned image and a separate
      // 4-byte copy of the error word).
      const size_t words = 3 * n + b->nq + 1;
      const size_t extra = stats ? (size_t)b->nq + ((b->d_blk_skip.p && b->launched) ? 2 * ((size_t)b->nq + 1) : 0) : 0;
      struct ImageLease {
        BufPool *pool;
        void *p = nullptr;
        size_t bytes = 0;
        ~ImageLease() {
          if (p) pool->give_image(p, bytes);
        }
      } lease{&ix->pool};
      std::vector<uint32_t> pageable;
      uint32_t *blk = nullptr;
      if ((words + extra) * 4 <= kPageableFetchBytes) {
        pageable.resize(words + extra);
        blk = pageable.data();
      } else {
        lease.p = ix->pool.take_image((words + extra) * 4, &lease.bytes);
        if (!lease.p) throw SlgError(SLG_ERR_OOM, "pinned staging image: hipHostMalloc failed");
        blk = static_cast<uint32_t *>(lease.p);
      }
      SLG_HIP(hipMemcpyAsync(blk, b->d_out.p, words * 4, hipMemcpyDeviceToHost, st));
      uint32_t *flagw = blk + words - 1;  // the index's error word as the batch's last kernel saw it
      uint32_t *const sblk = blk + words;
      if (stats) {
        SLG_HIP(hipMemcpyAsync(sblk, b->d_q_scored.p, (size_t)b->nq * 4, hipMemcpyDeviceToHost, st));
        if (b->d_blk_skip.p && b->launched)
          SLG_HIP(hipMemcpyAsync(sblk + b->nq, b->d_blk_skip.p, ((size_t)b->nq + 1) * 8, hipMemcpyDeviceToHost, st));
      }
      SLG_HIP(wait_stream(st));
      if (*flagw != 0u)
        throw SlgError(SLG_ERR_INTERNAL, "a scoring wave gave up on a round (chunk-loop guard): results are incomplete");
      if (n) {
        std::memcpy(out_doc, blk, n * 4);
        std::memcpy(out_seg, blk + n, n * 4);
        std::memcpy(out_score, blk + 2 * n, n * 4);
      }
      std::memcpy(out_count, blk + 3 * n, (size_t)b->nq * 4);
      if (stats) {
        scored.assign(sblk, sblk + b->nq);
        if (b->d_blk_skip.p && b->launched) {
          skipped.resize((size_t)b->nq + 1);
          std::memcpy(skipped.data(), sblk + b->nq, skipped.size() * 8);
        }
      }
    }
    if (stats)
      for (uint32_t q = 0; q < b->nq; q++) {
        // brute-force accounting: wand.rs:472 (postings_advanced += len), :500-503; with block
        // skipping, the postings that were never loaded are not counted as advanced over
        stats[q].postings_advanced = b->q_postings[q] - (skipped.empty() ? 0ull : skipped[q + 1]);
        stats[q].scored_docs = scored[q];
        stats[q].candidates_examined = scored[q];
      }
  });
}

int slg_batch_device_results(slg_batch *b, void **d_doc, void **d_seg, void **d_score,
                             void **d_count) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    if (d_doc) *d_doc = b->d_out_doc;
    if (d_seg) *d_seg = b->d_out_seg;
    if (d_score) *d_score = b->d_out_score;
    if (d_count) *d_count = b->d_out_count;
  });
}

int slg_batch_device_result_block(slg_batch *b, void **d_block, uint64_t *n_bytes) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    if (d_block) *d_block = b->d_out.p;
    if (n_bytes) *n_bytes = ((uint64_t)b->nq * b->k * 3 + b->nq) * 4;
  });
}

int slg_batch_info(const slg_batch *b, uint64_t *n_postings, uint32_t *n_slices,
                   uint64_t *algorithmic_bytes) {
  return guarded([&] {
    SLG_REQUIRE(b != nullptr, "batch is NULL");
    if (n_postings) *n_postings = b->n_postings;
    if (n_slices) *n_slices = b->n_slices;
    if (algorithmic_bytes) *algorithmic_bytes = 12ull * b->n_postings + 8ull * b->k * b->nq;
  });
}

int slg_batch_skip_counts(slg_batch *b, uint64_t *probed_postings, uint64_t *skipped_postings) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    DeviceGuard g(b->idx->device);
    unsigned long long c = 0ull;
    if (b->d_blk_skip.p) {
      SLG_HIP(hipStreamSynchronize(batch_stream(b)));
      SLG_HIP(hipMemcpy(&c, b->d_blk_skip.p, 8, hipMemcpyDeviceToHost));
    }
    if (probed_postings) *probed_postings = b->d_blk_skip.p ? b->n_postings_nonessential : 0ull;
    if (skipped_postings) *skipped_postings = c;
  });
}

#ifdef SLG_STAMPS
int slg_debug_read_stamps(slg_batch *b, unsigned long long *out, uint32_t n_slices) {
  return guarded([&] {
    SLG_HIP(hipStreamSynchronize(batch_stream(b)));
    SLG_HIP(hipMemcpy(out, b->d_stamps.p, (size_t)n_slices * 96, hipMemcpyDeviceToHost));
  });
}
#endif

int slg_batch_set_stream(slg_batch *b, void *hip_stream) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    slg_index *ix = b->idx;
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard g(ix->device);
    if (b->launched) SLG_HIP(hipStreamSynchronize(batch_stream(b)));  // queued work finishes first
    b->own_stream_set = hip_stream != SLG_OWN_STREAM;
    b->stream = b->own_stream_set ? (hipStream_t)hip_stream : nullptr;
  });
}

void slg_batch_destroy(slg_batch *b) {
  if (!b) return;
  slg_index *ix = b->idx;
  if (!ix) {  // detached by slg_index_destroy: nothing left on the device
    delete b;
    return;
  }
  int prev = -1;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(ix->device);
  hipStream_t st;
  {
    std::lock_guard<std::mutex> lk(ix->mu);
    st = batch_stream(b);
    auto it = std::find(ix->live.begin(), ix->live.end(), b);
    if (it != ix->live.end()) {
      *it = ix->live.back();
      ix->live.pop_back();
    }
  }
  (void)wait_stream(st);
  for (hipEvent_t e : b->ev_shard)
    if (e) (void)hipEventDestroy(e);
  delete b;
  if (prev >= 0) (void)hipSetDevice(prev);
}

int slg_search_batch(slg_index *ix, const slg_query *queries, uint32_t nq, uint32_t k,
                     int strategy, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                     uint32_t *out_count, slg_stats *stats) {
  return slg_search_batch_filtered(ix, queries, nq, nullptr, k, strategy, out_doc, out_seg, out_score,
                                   out_count, stats);
}

int slg_search_batch_filtered(slg_index *ix, const slg_query *queries, uint32_t nq,
                              const int32_t *q_filter, uint32_t k, int strategy, uint32_t *out_doc,
                              uint32_t *out_seg, float *out_score, uint32_t *out_count,
                              slg_stats *stats) {
  slg_batch *b = nullptr;
  int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(nq == 0 || queries != nullptr, "queries is NULL");
  });
  if (rc != SLG_OK) return rc;
  std::vector<uint32_t> offs(nq + 1, 0), tids;
  std::vector<float> ws;
  rc = guarded([&] {
    const size_t n_segs = ix->snapshot()->segs.size();
    for (uint32_t q = 0; q < nq; q++) {
      const slg_query &qq = queries[q];
      SLG_REQUIRE(qq.n_terms == 0 || (qq.term_ids && qq.weights), "query arrays are NULL");
      offs[q + 1] = offs[q] + qq.n_terms;
      tids.insert(tids.end(), qq.term_ids, qq.term_ids + (size_t)qq.n_terms * n_segs);
      ws.insert(ws.end(), qq.weights, qq.weights + qq.n_terms);
    }
  });
  if (rc != SLG_OK) return rc;
  b = slg_batch_prepare_filtered(ix, nq, offs.data(), tids.data(), ws.data(), q_filter, k, strategy);
  if (!b) return g_last_code;  // slg_batch_prepare set the thread-local error and its code
  rc = slg_batch_run(b);
  if (rc == SLG_OK) rc = slg_batch_fetch(b, out_doc, out_seg, out_score, out_count, stats);
  const std::string keep = g_last_error;
  slg_batch_destroy(b);
  g_last_error = keep;
  g_last_code = rc;
  return rc;
}

int slg_batch_matched_counts(slg_batch *b, uint64_t *out_matched) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->sorted || b->after, "not a sorted or cursor batch (slg_batch_prepare_sorted / _after)");
    SLG_REQUIRE(b->launched, "the batch has not run");
    SLG_REQUIRE(b->nq == 0 || out_matched != nullptr, "out_matched is NULL");
    slg_index *ix = b->idx;
    DeviceGuard g(ix->device);
    hipStream_t st;
    {
      std::lock_guard<std::mutex> lk(ix->mu);
      st = batch_stream(b);
    }
    SLG_HIP(wait_stream(st));
    if (b->nq) SLG_HIP(hipMemcpy(out_matched, b->d_matched.p, (size_t)b->nq * 8, hipMemcpyDeviceToHost));
  });
}

int slg_search_batch_sorted(slg_index *ix, const slg_query *queries, uint32_t nq, const slg_score_plans *plans,
                            const int32_t *q_filter, const slg_sort_spec *sort, uint32_t k, int strategy,
                            uint32_t *out_doc, uint32_t *out_seg, float *out_score, uint32_t *out_count,
                            uint64_t *out_matched) {
  int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(nq == 0 || queries != nullptr, "queries is NULL");
  });
  if (rc != SLG_OK) return rc;
  std::vector<uint32_t> offs(nq + 1, 0), tids;
  std::vector<float> ws;
  rc = guarded([&] {
    const size_t n_segs = ix->snapshot()->segs.size();
    for (uint32_t q = 0; q < nq; q++) {
      const slg_query &qq = queries[q];
      SLG_REQUIRE(qq.n_terms == 0 || (qq.term_ids && qq.weights), "query arrays are NULL");
      offs[q + 1] = offs[q] + qq.n_terms;
      tids.insert(tids.end(), qq.term_ids, qq.term_ids + (size_t)qq.n_terms * n_segs);
      ws.insert(ws.end(), qq.weights, qq.weights + qq.n_terms);
    }
  });
  if (rc != SLG_OK) return rc;
  slg_batch *b = slg_batch_prepare_sorted(ix, nq, offs.data(), tids.data(), ws.data(), plans, q_filter, sort, k,
                                          strategy);
  if (!b) return g_last_code;
  rc = slg_batch_run(b);
  if (rc == SLG_OK) rc = slg_batch_fetch(b, out_doc, out_seg, out_score, out_count, nullptr);
  if (rc == SLG_OK && out_matched) rc = slg_batch_matched_counts(b, out_matched);
  const std::string keep = g_last_error;
  slg_batch_destroy(b);
  g_last_error = keep;
  g_last_code = rc;
  return rc;
}

int slg_batch_cursor_seen(slg_batch *b, uint8_t *out_seen) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->after, "not a cursor batch (slg_batch_prepare_after)");
    SLG_REQUIRE(b->launched, "the batch has not run");
    SLG_REQUIRE(b->nq == 0 || out_seen != nullptr, "out_seen is NULL");
    slg_index *ix = b->idx;
    DeviceGuard g(ix->device);
    hipStream_t st;
    {
      std::lock_guard<std::mutex> lk(ix->mu);
      st = batch_stream(b);
    }
    SLG_HIP(wait_stream(st));
    std::vector<uint32_t> seen(b->nq);
    if (b->nq) SLG_HIP(hipMemcpy(seen.data(), b->d_seen.p, (size_t)b->nq * 4, hipMemcpyDeviceToHost));
    for (uint32_t q = 0; q < b->nq; q++) out_seen[q] = seen[q] ? 1u : 0u;
  });
}

int slg_search_batch_after(slg_index *ix, const slg_query *queries, uint32_t nq, const slg_score_plans *plans,
                           const int32_t *q_filter, const slg_sort_spec *sort, const slg_sort_cursor *q_cursor,
                           uint32_t k, int strategy, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                           uint32_t *out_count, uint64_t *out_matched, uint8_t *out_seen) {
  int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    SLG_REQUIRE(nq == 0 || queries != nullptr, "queries is NULL");
  });
  if (rc != SLG_OK) return rc;
  std::vector<uint32_t> offs(nq + 1, 0), tids;
  std::vector<float> ws;
  rc = guarded([&] {
    const size_t n_segs = ix->snapshot()->segs.size();
    for (uint32_t q = 0; q < nq; q++) {
      const slg_query &qq = queries[q];
      SLG_REQUIRE(qq.n_terms == 0 || (qq.term_ids && qq.weights), "query arrays are NULL");
      offs[q + 1] = offs[q] + qq.n_terms;
      tids.insert(tids.end(), qq.term_ids, qq.term_ids + (size_t)qq.n_terms * n_segs);
      ws.insert(ws.end(), qq.weights, qq.weights + qq.n_terms);
    }
  });
  if (rc != SLG_OK) return rc;
  slg_batch *b = slg_batch_prepare_after(ix, nq, offs.data(), tids.data(), ws.data(), plans, q_filter, sort,
                                         q_cursor, k, strategy);
  if (!b) return g_last_code;
  rc = slg_batch_run(b);
  if (rc == SLG_OK) rc = slg_batch_fetch(b, out_doc, out_seg, out_score, out_count, nullptr);
  if (rc == SLG_OK && out_matched) rc = slg_batch_matched_counts(b, out_matched);
  if (rc == SLG_OK && out_seen) rc = slg_batch_cursor_seen(b, out_seen);
  const std::string keep = g_last_error;
  slg_batch_destroy(b);
  g_last_error = keep;
  g_last_code = rc;
  return rc;
}

int slg_merge_shards_device(slg_index *ix, uint32_t n_shards, uint32_t nq, uint32_t k,
                            const uint32_t *d_doc, const uint32_t *d_seg, const float *d_score,
                            const uint32_t *d_count, uint32_t seg_stride, uint32_t *d_out_doc,
                            uint32_t *d_out_seg, float *d_out_score, uint32_t *d_out_count) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    if (k > SLG_MAX_K) throw SlgError(SLG_ERR_UNSUPPORTED, "k > SLG_MAX_K");
    if (nq == 0) return;
    SLG_REQUIRE(n_shards >= 1, "n_shards == 0");
    SLG_REQUIRE(d_count && d_out_count, "count arrays are NULL");
    SLG_REQUIRE(k == 0 || (d_doc && d_seg && d_score && d_out_doc && d_out_seg && d_out_score),
                "device arrays are NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard g(ix->device);
    if (k == 0) {
      SLG_HIP(hipMemsetAsync(d_out_count, 0, (size_t)nq * 4, ix->stream));
      return;
    }
    slg::ShardMergeParams mp{};
    mp.doc = d_doc;
    mp.seg = d_seg;
    mp.score = d_score;
    mp.count = d_count;
    mp.out_doc = d_out_doc;
    mp.out_seg = d_out_seg;
    mp.out_score = d_out_score;
    mp.out_count = d_out_count;
    mp.n_shards = n_shards;
    mp.nq = nq;
    mp.k = k;
    mp.seg_stride = seg_stride;
    mp.arr_stride = (uint64_t)nq * k;
    mp.cnt_stride = nq;
    launch_shard_merge(mp, ix->stream);
  });
}

// ---- index sharding over RCCL (api/reader.rs:2670-2778 with segment = shard) --------
// One process (or host thread) per GPU holds the segments of its shard; every rank scores the same
// query batch, ONE ncclAllGather exchanges the contiguous per-rank result blocks
// doc | seg | score | count ((3k+1) * Q * 4 bytes) over xGMI, and every rank merges the world's rows
// by (score desc, segment_ord asc, doc asc), segment_ord = rank * segs_per_rank + local segment
// (query/sort.rs:80-93).  RCCL is bound at run time (dlopen): a single-GPU user of the library does
// not need it, and inside a PyTorch process the librccl torch has loaded is the one used.
extern "C++" {
namespace {
typedef int (*nccl_get_uid_fn)(void *);
struct NcclUid {  // ncclUniqueId (rccl.h): passed to ncclCommInitRank BY VALUE
  char internal[128];
};
typedef int (*nccl_destroy_fn)(void *);
typedef int (*nccl_allgather_fn)(const void *, void *, size_t, int, void *, hipStream_t);
typedef const char *(*nccl_errstr_fn)(int);
struct RcclApi {
  void *handle = nullptr;
  nccl_get_uid_fn get_uid = nullptr;
  int (*init_rank)(void **, int, NcclUid, int) = nullptr;
  nccl_destroy_fn destroy = nullptr;
  nccl_allgather_fn allgather = nullptr;
  nccl_errstr_fn errstr = nullptr;
  std::string error;
};
RcclApi &rccl() {
  static RcclApi api = [] {
    RcclApi a;
    const char *names[] = {"librccl.so", "librccl.so.1"};
    for (const char *n : names)  // a copy that is already resident (PyTorch's) first
      if (!a.handle) a.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
    for (const char *n : {"librccl.so.1", "librccl.so"})
      if (!a.handle) a.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (!a.handle) {
      const char *e = dlerror();  // (one call: dlerror() clears the state it reports)
      a.error = std::string("librccl not found: ") + (e ? e : "");
      return a;
    }
    a.get_uid = (nccl_get_uid_fn)dlsym(a.handle, "ncclGetUniqueId");
    a.init_rank = (int (*)(void **, int, NcclUid, int))dlsym(a.handle, "ncclCommInitRank");
    a.destroy = (nccl_destroy_fn)dlsym(a.handle, "ncclCommDestroy");
    a.allgather = (nccl_allgather_fn)dlsym(a.handle, "ncclAllGather");
    a.errstr = (nccl_errstr_fn)dlsym(a.handle, "ncclGetErrorString");
    if (!a.get_uid || !a.init_rank || !a.destroy || !a.allgather || !a.errstr) a.error = "librccl lacks a required symbol";
    return a;
  }();
  if (!api.error.empty()) throw SlgError(SLG_ERR_UNSUPPORTED, api.error);
  return api;
}
void nccl_check(int rc, const char *what) {
  if (rc != 0) throw SlgError(SLG_ERR_DEVICE, std::string(what) + ": " + rccl().errstr(rc));
}
constexpr int kNcclInt32 = 2;  // ncclDataType_t ncclInt32 (rccl.h)
}  // namespace
}  // extern "C++"

struct slg_shard_group {
  slg_index *idx = nullptr;
  int rank = 0, world = 1;
  uint32_t segs_per_rank = 1;
  void *comm = nullptr;  // ncclComm_t
  // Collectives on one communicator must be issued in the same order on every rank.  The group owns
  // the stream they run on and hands out turns: sharded run number `seq` issues its all-gather when
  // the runs 0 .. seq-1 have issued theirs, whatever host thread or batch stream it comes from (the
  // batch's stream and the collective stream are tied together with events).
  hipStream_t coll_stream = nullptr;
  std::mutex mu;
  std::condition_variable cv;
  uint64_t next_seq = 0;   // the run whose collective may be issued next
  uint64_t auto_seq = 0;   // tickets of slg_batch_run_sharded (call order)
  // device time of the sharded runs fetched so far (slg_index profiling on): local kernels, all-gather
  // (incl. waiting for the slowest rank), merge; ms sums and the number of runs
  double ms_kernels = 0.0, ms_gather = 0.0, ms_merge = 0.0;
  uint64_t n_timed = 0;
};

int slg_shard_unique_id(void *out, size_t out_bytes) {
  return guarded([&] {
    SLG_REQUIRE(out != nullptr && out_bytes >= SLG_SHARD_UNIQUE_ID_BYTES, "unique id buffer is NULL or too small");
    NcclUid id;
    nccl_check(rccl().get_uid(&id), "ncclGetUniqueId");
    std::memcpy(out, id.internal, sizeof(id.internal));
  });
}

slg_shard_group *slg_shard_group_create(slg_index *ix, int rank, int world, const void *unique_id,
                                        uint32_t segs_per_rank) {
  slg_shard_group *g = nullptr;
  const int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr && unique_id != nullptr, "index or unique id is NULL");
    SLG_REQUIRE(world >= 1 && rank >= 0 && rank < world, "rank outside [0, world)");
    SLG_REQUIRE(segs_per_rank >= ix->snapshot()->segs.size(), "segs_per_rank is smaller than this shard's segment count");
    DeviceGuard dg(ix->device);
    NcclUid id;
    std::memcpy(id.internal, unique_id, sizeof(id.internal));
    g = new slg_shard_group();
    g->idx = ix;
    g->rank = rank;
    g->world = world;
    g->segs_per_rank = segs_per_rank;
    nccl_check(rccl().init_rank(&g->comm, world, id, rank), "ncclCommInitRank");
    SLG_HIP(hipStreamCreateWithFlags(&g->coll_stream, hipStreamNonBlocking));
  });
  if (rc != SLG_OK) {
    const std::string keep = g_last_error;
    delete g;
    g_last_error = keep;
    g_last_code = rc;
    return nullptr;
  }
  return g;
}

void slg_shard_group_destroy(slg_shard_group *g) {
  if (!g) return;
  if (g->comm) {
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(g->idx->device);
    (void)hipDeviceSynchronize();
    try {
      (void)rccl().destroy(g->comm);
    } catch (...) {
    }
    if (g->coll_stream) (void)hipStreamDestroy(g->coll_stream);
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  delete g;
}

namespace {
int run_sharded_impl(slg_batch *b, slg_shard_group *g, bool have_seq, uint64_t seq, uint32_t *out_doc,
                     uint32_t *out_seg, float *out_score, uint32_t *out_count) {
  int rc = guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(g != nullptr && g->idx == b->idx, "shard group is NULL or belongs to another index");
    SLG_REQUIRE(g->segs_per_rank >= b->snap->segs.size(), "the shard grew beyond the group's segs_per_rank");
    // (a cursor's segment_ord is index-global; the shard merge does not apply it)
    if (b->after) throw SlgError(SLG_ERR_UNSUPPORTED, "a cursor batch does not run sharded");
  });
  if (rc != SLG_OK) return rc;
  if (!have_seq) {  // call order = the order on every rank, if one thread issues the runs
    std::lock_guard<std::mutex> lk(g->mu);
    seq = g->auto_seq++;
  }
  slg_index *ix = b->idx;
  const bool timed = ix->profile;
  rc = guarded([&] {
    DeviceGuard dg(ix->device);
    for (int i = 0; i < 4; i++)
      if (!b->ev_shard[i]) SLG_HIP(hipEventCreateWithFlags(&b->ev_shard[i], timed ? hipEventDefault : hipEventDisableTiming));
    if (timed) {
      std::lock_guard<std::mutex> lk(ix->mu);
      SLG_HIP(hipEventRecord(b->ev_shard[0], batch_stream(b)));
    }
  });
  if (rc == SLG_OK) rc = slg_batch_run(b);  // this rank's segments: partition + score + merge, on the batch's stream
  // From here on the turn MUST be passed on, error or not: the runs behind this one wait for it.
  int rc2 = guarded([&] {
    const size_t n = (size_t)b->nq * b->k, blk = 3 * n + b->nq;  // words of one rank's block
    DeviceGuard dg(ix->device);
    hipStream_t st;
    {
      std::lock_guard<std::mutex> lk(ix->mu);
      st = batch_stream(b);
      if (rc == SLG_OK && b->nq) {
        if (!b->d_gather.p) b->d_gather.alloc_pooled(&ix->pool, (size_t)g->world * blk * 4);
        if (!b->d_merged.p) b->d_merged.alloc_pooled(&ix->pool, blk * 4);
        SLG_HIP(hipEventRecord(b->ev_shard[1], st));  // the local result block is complete
      }
    }
    {
      // my turn: ONE collective, every rank's contiguous block in rank order, on the group's stream
      std::unique_lock<std::mutex> lk(g->mu);
      g->cv.wait(lk, [&] { return g->next_seq == seq; });
      struct PassOn {
        slg_shard_group *g;
        std::unique_lock<std::mutex> &lk;
        ~PassOn() {
          g->next_seq++;
          lk.unlock();
          g->cv.notify_all();
        }
      } pass{g, lk};
      if (rc != SLG_OK || b->nq == 0) return;
      SLG_HIP(hipStreamWaitEvent(g->coll_stream, b->ev_shard[1], 0));
      nccl_check(rccl().allgather(b->d_out.p, b->d_gather.p, blk, kNcclInt32, g->comm, g->coll_stream), "ncclAllGather");
      SLG_HIP(hipEventRecord(b->ev_shard[2], g->coll_stream));
    }
    {
      std::lock_guard<std::mutex> lk(ix->mu);
      SLG_HIP(hipStreamWaitEvent(st, b->ev_shard[2], 0));
      uint32_t *m = b->d_merged.as<uint32_t>();
      const uint32_t *gb = b->d_gather.as<uint32_t>();
      if (b->k == 0) {
        SLG_HIP(hipMemsetAsync(m, 0, blk * 4, st));
      } else {
        slg::ShardMergeParams mp{};
        mp.doc = gb;
        mp.seg = gb + n;
        mp.score = reinterpret_cast<const float *>(gb + 2 * n);
        mp.count = gb + 3 * n;
        mp.out_doc = m;
        mp.out_seg = m + n;
        mp.out_score = reinterpret_cast<float *>(m + 2 * n);
        mp.out_count = m + 3 * n;
        mp.n_shards = (uint32_t)g->world;
        mp.nq = b->nq;
        mp.k = b->k;
        mp.seg_stride = g->segs_per_rank;
        mp.arr_stride = blk;
        mp.cnt_stride = blk;
        launch_shard_merge(mp, st);
      }
      if (timed) SLG_HIP(hipEventRecord(b->ev_shard[3], st));
      b->shard_group = g;
      b->shard_timed = timed;
    }
  });
  if (rc == SLG_OK) rc = rc2;
  // merged top-k to the caller's host arrays (else: slg_batch_fetch_sharded / _device_results later)
  if (rc == SLG_OK && out_count) rc = slg_batch_fetch_sharded(b, out_doc, out_seg, out_score, out_count);
  return rc;
}
}  // namespace

int slg_batch_run_sharded(slg_batch *b, slg_shard_group *g, uint32_t *out_doc, uint32_t *out_seg,
                          float *out_score, uint32_t *out_count) {
  return run_sharded_impl(b, g, false, 0, out_doc, out_seg, out_score, out_count);
}

int slg_batch_run_sharded_seq(slg_batch *b, slg_shard_group *g, uint64_t seq, uint32_t *out_doc, uint32_t *out_seg,
                              float *out_score, uint32_t *out_count) {
  return run_sharded_impl(b, g, true, seq, out_doc, out_seg, out_score, out_count);
}

int slg_shard_group_skip_seq(slg_shard_group *g, uint64_t seq) {
  return guarded([&] {
    SLG_REQUIRE(g != nullptr, "shard group is NULL");
    std::unique_lock<std::mutex> lk(g->mu);
    g->cv.wait(lk, [&] { return g->next_seq == seq; });
    g->next_seq++;
    lk.unlock();
    g->cv.notify_all();
  });
}

int slg_shard_group_stats(slg_shard_group *g, double *ms_kernels, double *ms_gather, double *ms_merge, uint64_t *n_runs) {
  return guarded([&] {
    SLG_REQUIRE(g != nullptr, "shard group is NULL");
    std::lock_guard<std::mutex> lk(g->mu);
    if (ms_kernels) *ms_kernels = g->ms_kernels;
    if (ms_gather) *ms_gather = g->ms_gather;
    if (ms_merge) *ms_merge = g->ms_merge;
    if (n_runs) *n_runs = g->n_timed;
    g->ms_kernels = g->ms_gather = g->ms_merge = 0.0;
    g->n_timed = 0;
  });
}

int slg_batch_fetch_sharded(slg_batch *b, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
                            uint32_t *out_count) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    if (b->after) throw SlgError(SLG_ERR_UNSUPPORTED, "a cursor batch does not run sharded");
    SLG_REQUIRE(b->nq == 0 || out_count != nullptr, "out_count is NULL");
    SLG_REQUIRE(b->nq == 0 || b->k == 0 || (out_doc && out_seg && out_score), "output array is NULL");
    if (b->nq == 0) return;
    SLG_REQUIRE(b->d_merged.p != nullptr, "slg_batch_run_sharded has not run on this batch");
    slg_index *ix = b->idx;
    DeviceGuard dg(ix->device);
    hipStream_t st;
    {
      std::lock_guard<std::mutex> lk(ix->mu);
      st = batch_stream(b);
    }
    const size_t n = (size_t)b->nq * b->k, blk = 3 * n + b->nq;
    struct ImageLease {  // pinned staging (see slg_batch_fetch)
      BufPool *pool;
      void *p = nullptr;
      size_t bytes = 0;
      ~ImageLease() {
        if (p) pool->give_image(p, bytes);
      }
    } lease{&ix->pool};
    lease.p = ix->pool.take_image(blk * 4, &lease.bytes);
    if (!lease.p) throw SlgError(SLG_ERR_OOM, "pinned staging image: hipHostMalloc failed");
    uint32_t *h = static_cast<uint32_t *>(lease.p);
    SLG_HIP(hipMemcpyAsync(h, b->d_merged.p, blk * 4, hipMemcpyDeviceToHost, st));
    SLG_HIP(wait_stream(st));
    if (b->shard_timed && b->shard_group) {  // device time of this run's three phases
      float k_ms = 0.0f, g_ms = 0.0f, m_ms = 0.0f;
      if (hipEventElapsedTime(&k_ms, b->ev_shard[0], b->ev_shard[1]) == hipSuccess &&
          hipEventElapsedTime(&g_ms, b->ev_shard[1], b->ev_shard[2]) == hipSuccess &&
          hipEventElapsedTime(&m_ms, b->ev_shard[2], b->ev_shard[3]) == hipSuccess) {
        std::lock_guard<std::mutex> lk(b->shard_group->mu);
        b->shard_group->ms_kernels += k_ms;
        b->shard_group->ms_gather += g_ms;
        b->shard_group->ms_merge += m_ms;
        b->shard_group->n_timed++;
      }
      b->shard_timed = false;
    }
    if (n) {
      std::memcpy(out_doc, h, n * 4);
      std::memcpy(out_seg, h + n, n * 4);
      std::memcpy(out_score, h + 2 * n, n * 4);
    }
    std::memcpy(out_count, h + 3 * n, (size_t)b->nq * 4);
  });
}

int slg_batch_sharded_device_results(slg_batch *b, void **d_doc, void **d_seg, void **d_score, void **d_count) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->d_merged.p != nullptr || b->nq == 0, "slg_batch_run_sharded has not run on this batch");
    const size_t n = (size_t)b->nq * b->k;
    uint32_t *m = b->d_merged.as<uint32_t>();
    if (d_doc) *d_doc = m;
    if (d_seg) *d_seg = m ? m + n : nullptr;
    if (d_score) *d_score = m ? m + 2 * n : nullptr;
    if (d_count) *d_count = m ? m + 3 * n : nullptr;
  });
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

namespace {
// dimension / metric / device stores of vector field f (0: the field of the segment descriptors;
// mixed_metric: its segments may differ in metric — the single-clause kernel reads it per segment —
// and *metric is the last one's)
void field_facts(const IndexState &S, uint32_t f, uint32_t *dim, int32_t *metric, const slg::VecSegDev **vsegs,
                 bool mixed_metric = false) {
  if (f == 0) {
    uint32_t d = 0;
    int32_t m = -1;
    for (auto &s : S.segs) {
      if (!s->store->vec_dim) continue;
      SLG_REQUIRE(d == 0 || d == s->store->vec_dim, "segments disagree on vec_dim");
      SLG_REQUIRE(mixed_metric || m < 0 || m == s->store->vec_metric, "segments disagree on the vector metric");
      d = s->store->vec_dim;
      m = s->store->vec_metric;
    }
    if (d == 0) throw SlgError(SLG_ERR_UNSUPPORTED, "index has no vector field");
    *dim = d;
    *metric = m;
    *vsegs = S.d_vsegs.as<slg::VecSegDev>();
    return;
  }
  SLG_REQUIRE(f <= S.vfields.size(), "unknown vector field id");
  const VecFieldHost &vf = *S.vfields[f - 1];
  *dim = vf.dim;
  *metric = vf.metric;
  *vsegs = vf.d_vsegs.as<slg::VecSegDev>();
}

enum class RerankShape { One, Multi, Fields };  // rerank_kernel, rerank_multi_kernel, rerank_fields_kernel

// One rerank call, checked against one snapshot of the index.  fp holds the parameters of every
// shape (the fields kernel's are a superset): base, boost, n_clauses, q_floats = the floats of one
// query's clause vectors; the per-clause tables are the fields shape's only.
struct RerankCall {
  std::shared_ptr<const IndexState> S;  // (a retired state waits for the device before its tables go)
  RerankShape shape = RerankShape::One;
  slg::RerankFieldsParams fp{};
};

// The host-only step of every rerank entry: all checks, in one order for the host and device forms,
// then the kernel facts of the call's shape.  io's pointers are only tested for NULL (mem names
// their memory in the message).  false: nq == 0, nothing to do.  Multi-clause entries with one
// clause and no boost take the single-clause kernel, which has no n_clauses check.
bool rerank_prepare(slg_index *ix, bool fields, uint32_t n_clauses, const uint32_t *clause_field, const float *boost,
                    const slg::RerankParams &io, const char *mem, RerankCall *rc) {
  if (fields)
    SLG_REQUIRE(ix != nullptr && clause_field != nullptr, "index or clause_field is NULL");
  else
    SLG_REQUIRE(ix != nullptr, "index is NULL");
  rc->shape = fields ? RerankShape::Fields
                     : (n_clauses == 1 && boost == nullptr ? RerankShape::One : RerankShape::Multi);
  if (rc->shape != RerankShape::One && (n_clauses < 1 || n_clauses > SLG_MAX_VECTOR_CLAUSES))
    throw SlgError(SLG_ERR_UNSUPPORTED, "n_clauses outside 1..SLG_MAX_VECTOR_CLAUSES");
  if (io.k_out > SLG_MAX_RERANK_K) throw SlgError(SLG_ERR_UNSUPPORTED, "k_out > SLG_MAX_RERANK_K");
  if (io.nq == 0) return false;
  SLG_REQUIRE(io.qvecs && io.alpha && io.cand_count && io.out_count, std::string(mem) + " arrays are NULL");
  SLG_REQUIRE(io.max_cand == 0 || (io.cand_doc && io.cand_seg && io.cand_bm25), "candidate arrays are NULL");
  SLG_REQUIRE(io.k_out == 0 || (io.out_doc && io.out_seg && io.out_score), "output arrays are NULL");
  rc->S = ix->snapshot();
  const IndexState &S = *rc->S;
  slg::RerankFieldsParams &fp = rc->fp;
  fp.base = io;
  fp.base.n_segs = (uint32_t)S.segs.size();
  fp.boost = boost;
  fp.n_clauses = n_clauses;
  if (rc->shape == RerankShape::Fields) {
    for (uint32_t c = 0; c < n_clauses; c++) {
      field_facts(S, clause_field[c], &fp.cdim[c], &fp.cmetric[c], &fp.cvsegs[c]);
      fp.coff[c] = fp.q_floats;
      fp.q_floats += fp.cdim[c];
    }
    if (slg::rerank_fields_lds_floats(n_clauses, fp.q_floats, io.max_cand) > slg::kRerankMultiLdsFloats)
      throw SlgError(SLG_ERR_UNSUPPORTED, "clause vectors + n_clauses * max_cand exceed the LDS budget of the rerank");
    return true;
  }
  int32_t metric;
  field_facts(S, 0, &fp.base.dim, &metric, &fp.base.vsegs, rc->shape == RerankShape::One);
  fp.base.metric = metric;
  fp.q_floats = n_clauses * fp.base.dim;
  if (rc->shape == RerankShape::One) {
    if (io.max_cand > slg::kRerankMaxCand)
      throw SlgError(SLG_ERR_UNSUPPORTED, "max_cand > " + std::to_string(slg::kRerankMaxCand));
    return true;
  }
  for (auto &s : S.segs)
    if (!s->store->vec_dim) throw SlgError(SLG_ERR_UNSUPPORTED, "multi-clause rerank needs the vector field in every segment");
  if (slg::rerank_multi_lds_floats(n_clauses, fp.base.dim, io.max_cand) > slg::kRerankMultiLdsFloats)
    throw SlgError(SLG_ERR_UNSUPPORTED, "n_clauses * (dim + max_cand) exceeds the LDS budget of the multi-clause rerank");
  return true;
}

// The launch step: the kernel of the call's shape on st, with the device pointers of rc.fp (the
// caller holds ix->mu and the device)
void rerank_launch(const RerankCall &rc, hipStream_t st) {
  const slg::RerankFieldsParams &fp = rc.fp;
  const int kregs = kregs_for(fp.base.k_out ? fp.base.k_out : 1);
  if (rc.shape == RerankShape::One) {
    SLG_HIP(slg::launch_rerank(fp.base, kregs, st));
  } else if (rc.shape == RerankShape::Multi) {
    const slg::RerankMultiParams mp{fp.base, fp.boost, fp.n_clauses, fp.base.dim + 4};
    SLG_HIP(slg::launch_rerank_multi(mp, kregs, st));
  } else {
    SLG_HIP(slg::launch_rerank_fields(fp, kregs, st));
  }
}

// The _device entries: device arrays in and out, asynchronous on the index stream or, b set, on the
// batch's (read under ix->mu, with the launch)
void rerank_device(slg_index *ix, const slg_batch *b, bool fields, uint32_t n_clauses, const uint32_t *clause_field,
                   const float *d_boost, const slg::RerankParams &d) {
  RerankCall rc;
  if (!rerank_prepare(ix, fields, n_clauses, clause_field, d_boost, d, "device", &rc)) return;
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  rerank_launch(rc, b ? batch_stream(b) : ix->stream);
}

// waits for a stream when it goes out of scope
struct StreamSync {
  hipStream_t st;
  ~StreamSync() { (void)hipStreamSynchronize(st); }
};

// The host-array entries: checks first, then pooled device buffers, H2D, launch, D2H and a wait, all on
// the index stream.  Declared after the buffers, `done` waits for the stream on every exit, so no
// block goes back to the pool while a queued copy or kernel may still use it.
void rerank_staged(slg_index *ix, bool fields, uint32_t n_clauses, const uint32_t *clause_field, const float *boost,
                   const slg::RerankParams &h) {
  RerankCall rc;
  if (!rerank_prepare(ix, fields, n_clauses, clause_field, boost, h, "host", &rc)) return;
  const size_t nq = h.nq, nqc = nq * n_clauses, nc = nq * h.max_cand, no = nq * h.k_out;
  DeviceGuard g(ix->device);
  const hipStream_t st = ix->stream;
  DevBuf dq, da, db, dcd, dcs, dcb, dcc, dod, dos, dosc, dov, doc_;
  StreamSync done{st};
  const auto up = [&](DevBuf &buf, const void *src, size_t n) -> DevBuf & {
    buf.alloc_pooled(&ix->pool, n * 4);
    if (src && n) SLG_HIP(hipMemcpyAsync(buf.p, src, n * 4, hipMemcpyHostToDevice, st));
    return buf;
  };
  slg::RerankParams &d = rc.fp.base;
  d.qvecs = up(dq, h.qvecs, nq * rc.fp.q_floats).as<float>();
  d.alpha = up(da, h.alpha, nqc).as<float>();
  if (boost) rc.fp.boost = up(db, boost, nqc).as<float>();
  d.cand_doc = up(dcd, h.cand_doc, nc).as<uint32_t>();
  d.cand_seg = up(dcs, h.cand_seg, nc).as<uint32_t>();
  d.cand_bm25 = up(dcb, h.cand_bm25, nc).as<float>();
  d.cand_count = up(dcc, h.cand_count, nq).as<uint32_t>();
  d.out_doc = up(dod, nullptr, no).as<uint32_t>();
  d.out_seg = up(dos, nullptr, no).as<uint32_t>();
  d.out_score = up(dosc, nullptr, no).as<float>();
  d.out_vec = up(dov, nullptr, no).as<float>();
  d.out_count = up(doc_, nullptr, nq).as<uint32_t>();
  {
    std::lock_guard<std::mutex> lk(ix->mu);
    rerank_launch(rc, st);
  }
  const auto down = [&](void *dst, const void *src, size_t n) {
    if (dst && n) SLG_HIP(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToHost, st));
  };
  down(h.out_doc, d.out_doc, no);
  down(h.out_seg, d.out_seg, no);
  down(h.out_score, d.out_score, no);
  down(h.out_vec, d.out_vec, no);
  down(h.out_count, d.out_count, nq);
  SLG_HIP(hipStreamSynchronize(st));
}
}  // namespace

int slg_rerank_batch_device(slg_index *ix, uint32_t nq, const float *d_qvecs, const float *d_alpha,
                            const uint32_t *d_cand_doc, const uint32_t *d_cand_seg,
                            const float *d_cand_bm25, const uint32_t *d_cand_count,
                            uint32_t max_cand, uint32_t k_out, uint32_t *d_out_doc,
                            uint32_t *d_out_seg, float *d_out_score, float *d_out_vec_score,
                            uint32_t *d_out_count) {
  return slg_rerank_multi_batch_device(ix, nq, 1, d_qvecs, d_alpha, nullptr, d_cand_doc, d_cand_seg, d_cand_bm25,
                                       d_cand_count, max_cand, k_out, d_out_doc, d_out_seg, d_out_score,
                                       d_out_vec_score, d_out_count);
}

int slg_rerank_multi_batch_device(slg_index *ix, uint32_t nq, uint32_t n_clauses, const float *d_qvecs,
                                  const float *d_alpha, const float *d_boost, const uint32_t *d_cand_doc,
                                  const uint32_t *d_cand_seg, const float *d_cand_bm25,
                                  const uint32_t *d_cand_count, uint32_t max_cand, uint32_t k_out,
                                  uint32_t *d_out_doc, uint32_t *d_out_seg, float *d_out_score,
                                  float *d_out_vec_score, uint32_t *d_out_count) {
  return guarded([&] {
    rerank_device(ix, nullptr, false, n_clauses, nullptr, d_boost,
                  {nullptr, 0, 0, d_qvecs, d_alpha, d_cand_doc, d_cand_seg, d_cand_bm25, d_cand_count, max_cand,
                   k_out, d_out_doc, d_out_seg, d_out_score, d_out_vec_score, d_out_count, nq});
  });
}

int slg_batch_rerank_device(slg_batch *b, uint32_t n_clauses, const float *d_qvecs, const float *d_alpha,
                            const float *d_boost, uint32_t k_out, uint32_t *d_out_doc, uint32_t *d_out_seg,
                            float *d_out_score, float *d_out_vec_score, uint32_t *d_out_count) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    rerank_device(b->idx, b, false, n_clauses, nullptr, d_boost,
                  {nullptr, 0, 0, d_qvecs, d_alpha, b->d_out_doc, b->d_out_seg, b->d_out_score, b->d_out_count,
                   b->k, k_out, d_out_doc, d_out_seg, d_out_score, d_out_vec_score, d_out_count, b->nq});
  });
}

int slg_rerank_fields_batch_device(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                                   const float *d_qvecs, const float *d_alpha, const float *d_boost,
                                   const uint32_t *d_cand_doc, const uint32_t *d_cand_seg,
                                   const float *d_cand_bm25, const uint32_t *d_cand_count, uint32_t max_cand,
                                   uint32_t k_out, uint32_t *d_out_doc, uint32_t *d_out_seg, float *d_out_score,
                                   float *d_out_vec_score, uint32_t *d_out_count) {
  return guarded([&] {
    rerank_device(ix, nullptr, true, n_clauses, clause_field, d_boost,
                  {nullptr, 0, 0, d_qvecs, d_alpha, d_cand_doc, d_cand_seg, d_cand_bm25, d_cand_count, max_cand,
                   k_out, d_out_doc, d_out_seg, d_out_score, d_out_vec_score, d_out_count, nq});
  });
}

int slg_rerank_fields_batch(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                            const float *qvecs, const float *alpha, const float *boost,
                            const uint32_t *cand_doc, const uint32_t *cand_seg, const float *cand_bm25,
                            const uint32_t *cand_count, uint32_t max_cand, uint32_t k_out, uint32_t *out_doc,
                            uint32_t *out_seg, float *out_score, float *out_vec_score, uint32_t *out_count) {
  return guarded([&] {
    rerank_staged(ix, true, n_clauses, clause_field, boost,
                  {nullptr, 0, 0, qvecs, alpha, cand_doc, cand_seg, cand_bm25, cand_count, max_cand, k_out, out_doc,
                   out_seg, out_score, out_vec_score, out_count, nq});
  });
}

int slg_rerank_multi_batch(slg_index *ix, uint32_t nq, uint32_t n_clauses, const float *qvecs,
                           const float *alpha, const float *boost, const uint32_t *cand_doc,
                           const uint32_t *cand_seg, const float *cand_bm25, const uint32_t *cand_count,
                           uint32_t max_cand, uint32_t k_out, uint32_t *out_doc, uint32_t *out_seg,
                           float *out_score, float *out_vec_score, uint32_t *out_count) {
  return guarded([&] {
    rerank_staged(ix, false, n_clauses, nullptr, boost,
                  {nullptr, 0, 0, qvecs, alpha, cand_doc, cand_seg, cand_bm25, cand_count, max_cand, k_out, out_doc,
                   out_seg, out_score, out_vec_score, out_count, nq});
  });
}

int slg_rerank_batch(slg_index *ix, uint32_t nq, const float *qvecs, const float *alpha,
                     const uint32_t *cand_doc, const uint32_t *cand_seg, const float *cand_bm25,
                     const uint32_t *cand_count, uint32_t max_cand, uint32_t k_out,
                     uint32_t *out_doc, uint32_t *out_seg, float *out_score, float *out_vec_score,
                     uint32_t *out_count) {
  return slg_rerank_multi_batch(ix, nq, 1, qvecs, alpha, nullptr, cand_doc, cand_seg, cand_bm25, cand_count,
                                max_cand, k_out, out_doc, out_seg, out_score, out_vec_score, out_count);
}

int slg_index_add_vector_field(slg_index *ix, const slg_vector_field_desc *per_segment, uint32_t n_segs) {
  int id = 0;
  const int rc = guarded([&] {
    SLG_REQUIRE(ix != nullptr && per_segment != nullptr, "index or descriptors are NULL");
    std::lock_guard<std::mutex> ulk(ix->update_mu);
    const auto cur = ix->snapshot();
    SLG_REQUIRE(n_segs == cur->segs.size(), "one descriptor per segment of the index is required");
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
      const uint32_t nd = cur->segs[s]->n_docs;
      for (uint32_t i = 0; i < nd; i++)
        SLG_REQUIRE(d.vec_offsets[i] == SLG_NO_VECTOR || d.vec_offsets[i] < d.vec_rows, "vector offset past vec_rows");
    }
    SLG_REQUIRE(vf->dim != 0, "no segment has vectors in this field");
    DeviceGuard g(ix->device);
    vf->per_seg.resize(n_segs);
    for (uint32_t s = 0; s < n_segs; s++) {
      const slg_vector_field_desc &d = per_segment[s];
      if (!d.vec_dim) continue;
      auto vs = std::make_shared<VecSegStore>();
      const size_t ob = (size_t)cur->segs[s]->n_docs * 4, vb = (size_t)d.vec_rows * d.vec_dim * 4;
      vs->offsets.alloc(ob, &ix->pool);
      if (ob) SLG_HIP(hipMemcpy(vs->offsets.p, d.vec_offsets, ob, hipMemcpyHostToDevice));
      vs->values.alloc(vb, &ix->pool);
      if (vb) SLG_HIP(hipMemcpy(vs->values.p, d.vec_values, vb, hipMemcpyHostToDevice));
      vs->dim = d.vec_dim;
      vf->per_seg[s] = std::move(vs);
    }
    auto ns = copy_state(*cur);
    ns->generation = cur->generation;
    ns->vfields.push_back(std::move(vf));
    finish_state(ix, *ns);
    id = (int)ns->vfields.size();
    publish(ix, std::move(ns));
  });
  return rc == SLG_OK ? id : rc;
}

}  // extern "C"

// ---- exact vector-only search (slg_vector_search_batch*, slg_vsearch.hpp) ----------------------
namespace {

// One call, checked against one snapshot of the index: every check runs before any device work
struct VsCall {
  std::shared_ptr<const IndexState> S;
  uint32_t nq = 0, n_clauses = 0, cand = 0, k_out = 0;
  uint32_t dim[SLG_MAX_VECTOR_CLAUSES] = {}, coff[SLG_MAX_VECTOR_CLAUSES] = {};
  int32_t metric[SLG_MAX_VECTOR_CLAUSES] = {};
  const slg::VecSegDev *vsegs[SLG_MAX_VECTOR_CLAUSES] = {};
  uint32_t q_floats = 0;
};

// The arrays of one call (host or device memory, as the entry says)
struct VsArgs {
  const float *qvecs, *alpha, *boost;
  const int32_t *q_filter;
  uint32_t *out_doc, *out_seg;
  float *out_score, *out_vec;
  uint32_t *out_count;
  uint64_t *out_total;
};

// false: nq == 0, nothing to do.  host_filter: q_filter is host memory and its ids are checked here
bool vs_prepare(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field, uint32_t cand_size,
                uint32_t k_out, const VsArgs &a, bool host_filter, VsCall *vc) {
  SLG_REQUIRE(ix != nullptr && clause_field != nullptr, "index or clause_field is NULL");
  if (n_clauses < 1 || n_clauses > SLG_MAX_VECTOR_CLAUSES)
    throw SlgError(SLG_ERR_UNSUPPORTED, "n_clauses outside 1..SLG_MAX_VECTOR_CLAUSES");
  if (cand_size < 1 || cand_size > SLG_MAX_VECTOR_CANDIDATES)
    throw SlgError(SLG_ERR_UNSUPPORTED, "cand_size outside 1..SLG_MAX_VECTOR_CANDIDATES");
  if (k_out > SLG_MAX_K) throw SlgError(SLG_ERR_UNSUPPORTED, "k_out > SLG_MAX_K");
  if (nq == 0) return false;
  SLG_REQUIRE(a.qvecs && a.alpha && a.out_count && a.out_total, "query or count arrays are NULL");
  SLG_REQUIRE(k_out == 0 || (a.out_doc && a.out_seg && a.out_score), "output arrays are NULL");
  vc->S = ix->snapshot();
  const IndexState &S = *vc->S;
  SLG_REQUIRE(S.total_docs < 0xFFFFFFFFull, "more than 2^32 - 2 docs in the index");
  vc->nq = nq;
  vc->n_clauses = n_clauses;
  vc->cand = cand_size;
  vc->k_out = k_out;
  for (uint32_t c = 0; c < n_clauses; c++) {
    field_facts(S, clause_field[c], &vc->dim[c], &vc->metric[c], &vc->vsegs[c]);
    vc->coff[c] = vc->q_floats;
    vc->q_floats += vc->dim[c];
  }
  if (host_filter && a.q_filter)
    for (uint32_t q = 0; q < nq; q++) {
      const int32_t f = a.q_filter[q];
      if (f < 0) continue;
      SLG_REQUIRE((size_t)f < S.filters.size() && S.filters[f] && S.filters[f]->complete() &&
                      S.filters[f]->per_seg.size() == S.segs.size(),
                  "q_filter names no filter registered for every segment");
    }
  return true;
}

template <typename K, typename P>
void vs_launch_kernel(K kernel, const P &params, dim3 grid, uint32_t threads, size_t lds, hipStream_t st) {
  if (lds > 48 * 1024)
    SLG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
  hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, st, params);
  SLG_HIP(hipGetLastError());
}

// the kernels of one call on st, device arrays in a (the caller holds ix->mu and the device)
void vs_run(slg_index *ix, const VsCall &vc, const VsArgs &a, hipStream_t st) {
  const IndexState &S = *vc.S;
  const uint32_t nq = vc.nq, NC = vc.n_clauses, K = vc.cand;
  const uint32_t n_segs = (uint32_t)S.segs.size();
  const uint64_t n_tiles64 = (S.total_docs + slg::kVsTileDocs - 1) / slg::kVsTileDocs;
  const uint32_t n_tiles = (uint32_t)n_tiles64;
  const uint32_t qtiles = (nq + slg::kVsTileQ - 1) / slg::kVsTileQ;
  const bool small = K <= slg::kVsSmallK;
  // the path is chosen from cand_size: small = fused top-k epilogue, else chunks of docs + select
  uint32_t n_chunks = 0, tpb = 0, chunk_docs = 0;
  const uint32_t cap = K <= slg::kVsSmallK / 2 ? slg::kVsBufCapNarrow : slg::kVsBufCap;
  if (small && n_tiles) {
    // one round of resident workgroups: as many as the LDS of a CU holds (at most 3, the VGPR bound)
    int n_cu = 0;
    SLG_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ix->device));
    const uint32_t per_cu = std::min<uint32_t>(3u, (uint32_t)((160u << 10) / slg::vs_scan_lds_bytes(true, cap)));
    const uint32_t target = std::max<uint32_t>((uint32_t)n_cu, 1u) * std::max<uint32_t>(per_cu, 1u);
    n_chunks = std::min<uint32_t>(std::max<uint32_t>((target + qtiles - 1) / qtiles, 1u),
                                  std::min<uint32_t>(n_tiles, (slg::kVsSortCap - slg::kVsSmallK) / slg::kVsSmallK));
    tpb = (n_tiles + n_chunks - 1) / n_chunks;
    n_chunks = (n_tiles + tpb - 1) / tpb;
  } else if (!small) {
    chunk_docs = ((slg::kVsSortCap - K) / slg::kVsTileDocs) * slg::kVsTileDocs;
  }
  const size_t n_run = (size_t)NC * nq * K;
  const size_t n_in = small ? (size_t)NC * nq * n_chunks * slg::kVsSmallK : (size_t)nq * chunk_docs;
  const uint32_t P = slg::vs_pow2(NC * K);
  const size_t n_u = P > slg::kVsSortCap ? (size_t)nq * P : 0;
  const size_t bytes = (2 * n_run + std::max<size_t>(n_in, 1) + n_u) * 8 + (size_t)NC * nq * 4 + 256;
  if (ix->vs_scratch.bytes < bytes) ix->vs_scratch.alloc(bytes + bytes / 4, &ix->pool);
  uint64_t *run = ix->vs_scratch.as<uint64_t>(), *dlist = run + n_run, *in = dlist + n_run;
  uint64_t *ukeys = in + std::max<size_t>(n_in, 1);
  uint32_t *run_cnt = reinterpret_cast<uint32_t *>(ukeys + n_u);
  SLG_HIP(hipMemsetAsync(run_cnt, 0, (size_t)NC * nq * 4, st));

  slg::VsScanParams sp{};
  sp.segs = S.d_segs.as<slg::SegDev>();
  sp.reject_table = S.d_reject_table.as<const uint32_t *>();
  sp.doc_base = S.d_doc_base.as<uint32_t>();
  sp.n_segs = n_segs;
  sp.n_filters = (uint32_t)S.filters.size();
  sp.nq = nq;
  sp.qvecs = a.qvecs;
  sp.q_stride = vc.q_floats;
  sp.boost = a.boost;
  sp.n_clauses = NC;
  sp.q_filter = a.q_filter;
  sp.k = K;
  sp.cap = cap;
  auto scan = [&](uint32_t c, bool topk, dim3 grid) {
    sp.vsegs = vc.vsegs[c];
    sp.dim = vc.dim[c];
    sp.q_off = vc.coff[c];
    sp.clause = c;
    sp.qvec4 = (vc.q_floats % 4 == 0 && vc.coff[c] % 4 == 0 && ((uintptr_t)a.qvecs & 15) == 0) ? 1u : 0u;
    const size_t lds = slg::vs_scan_lds_bytes(topk, sp.cap);
    if (vc.metric[c] == 0)
      topk ? vs_launch_kernel(slg::vs_scan_kernel<0, true>, sp, grid, 256, lds, st)
           : vs_launch_kernel(slg::vs_scan_kernel<0, false>, sp, grid, 256, lds, st);
    else
      topk ? vs_launch_kernel(slg::vs_scan_kernel<1, true>, sp, grid, 256, lds, st)
           : vs_launch_kernel(slg::vs_scan_kernel<1, false>, sp, grid, 256, lds, st);
  };
  slg::VsSelectParams sel{};
  sel.run = run;
  sel.run_cnt = run_cnt;
  sel.dlist = dlist;
  sel.nq = nq;
  sel.k = K;
  sel.in = in;
  auto select = [&](uint32_t c0, uint32_t n_cl, uint32_t n_in_q, uint32_t stride, bool final_) {
    sel.c0 = c0;
    sel.n_in = n_in_q;
    sel.in_stride = stride;
    sel.final_ = final_ ? 1u : 0u;
    const size_t lds = (size_t)slg::vs_pow2(K + n_in_q) * 8;
    vs_launch_kernel(slg::vs_select_kernel, sel, dim3(nq, n_cl), slg::kVsSortThreads, lds, st);
  };
  if (small) {
    sp.tile_begin = 0;
    sp.tile_end = n_tiles;
    sp.tiles_per_block = tpb;
    sp.n_chunks = n_chunks;
    for (uint32_t c = 0; c < NC && n_chunks; c++) {
      sp.out = in + (size_t)c * nq * n_chunks * slg::kVsSmallK;
      scan(c, true, dim3(qtiles, n_chunks));
    }
    select(0, NC, n_chunks * slg::kVsSmallK, n_chunks * slg::kVsSmallK, true);
  } else {
    const uint32_t tiles_per_chunk = chunk_docs / slg::kVsTileDocs;
    sp.out = in;
    sp.out_stride = chunk_docs;
    sp.tiles_per_block = 1;
    const uint32_t steps = std::max<uint32_t>((n_tiles + tiles_per_chunk - 1) / tiles_per_chunk, 1u);
    for (uint32_t s = 0; s < steps; s++) {
      const uint32_t t0 = s * tiles_per_chunk, t1 = std::min<uint32_t>(t0 + tiles_per_chunk, n_tiles);
      sp.tile_begin = t0;
      sp.tile_end = t1;
      for (uint32_t c = 0; c < NC; c++) {
        if (t1 > t0) scan(c, false, dim3(qtiles, t1 - t0));
        select(c, 1, (t1 > t0 ? t1 - t0 : 0) * slg::kVsTileDocs, chunk_docs, s + 1 == steps);
      }
    }
  }
  slg::VsBlendParams bp{};
  bp.dlist = dlist;
  bp.run_cnt = run_cnt;
  bp.nq = nq;
  bp.k = K;
  bp.n_clauses = NC;
  bp.alpha = a.alpha;
  for (uint32_t c = 0; c < NC; c++) bp.metric[c] = vc.metric[c];
  bp.doc_base = S.d_doc_base.as<uint32_t>();
  bp.n_segs = n_segs;
  bp.ukeys = ukeys;
  bp.P = P;
  bp.k_out = vc.k_out;
  bp.out_doc = a.out_doc;
  bp.out_seg = a.out_seg;
  bp.out_score = a.out_score;
  bp.out_vec = a.out_vec;
  bp.out_count = a.out_count;
  bp.out_total = a.out_total;
  vs_launch_kernel(slg::vs_blend_kernel, bp, dim3(nq), slg::kVsSortThreads,
                   P > slg::kVsSortCap ? 0 : (size_t)P * 8, st);
}

void vs_device(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field, uint32_t cand_size,
               uint32_t k_out, const VsArgs &d) {
  VsCall vc;
  if (!vs_prepare(ix, nq, n_clauses, clause_field, cand_size, k_out, d, false, &vc)) return;
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  vs_run(ix, vc, d, ix->stream);
}

// host arrays: checks, pooled device buffers, H2D, the kernels, D2H and a wait, all on the index stream
// (as rerank_staged)
void vs_staged(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field, uint32_t cand_size,
               uint32_t k_out, const VsArgs &h) {
  VsCall vc;
  if (!vs_prepare(ix, nq, n_clauses, clause_field, cand_size, k_out, h, true, &vc)) return;
  const size_t nqc = (size_t)nq * n_clauses, no = (size_t)nq * k_out;
  DeviceGuard g(ix->device);
  const hipStream_t st = ix->stream;
  DevBuf dq, da, db, df, dod, dos, dosc, dov, doc_, dot;
  StreamSync done{st};
  const auto up = [&](DevBuf &buf, const void *src, size_t bytes) -> DevBuf & {
    buf.alloc_pooled(&ix->pool, bytes);
    if (src && bytes) SLG_HIP(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, st));
    return buf;
  };
  VsArgs d{};
  d.qvecs = up(dq, h.qvecs, (size_t)nq * vc.q_floats * 4).as<float>();
  d.alpha = up(da, h.alpha, nqc * 4).as<float>();
  if (h.boost) d.boost = up(db, h.boost, nqc * 4).as<float>();
  if (h.q_filter) d.q_filter = up(df, h.q_filter, (size_t)nq * 4).as<int32_t>();
  d.out_doc = up(dod, nullptr, no * 4).as<uint32_t>();
  d.out_seg = up(dos, nullptr, no * 4).as<uint32_t>();
  d.out_score = up(dosc, nullptr, no * 4).as<float>();
  d.out_vec = up(dov, nullptr, no * 4).as<float>();
  d.out_count = up(doc_, nullptr, (size_t)nq * 4).as<uint32_t>();
  d.out_total = up(dot, nullptr, (size_t)nq * 8).as<uint64_t>();
  {
    std::lock_guard<std::mutex> lk(ix->mu);
    vs_run(ix, vc, d, st);
  }
  const auto down = [&](void *dst, const void *src, size_t bytes) {
    if (dst && bytes) SLG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
  };
  down(h.out_doc, d.out_doc, no * 4);
  down(h.out_seg, d.out_seg, no * 4);
  down(h.out_score, d.out_score, no * 4);
  down(h.out_vec, d.out_vec, no * 4);
  down(h.out_count, d.out_count, (size_t)nq * 4);
  down(h.out_total, d.out_total, (size_t)nq * 8);
  SLG_HIP(hipStreamSynchronize(st));
}
}  // namespace

extern "C" {

int slg_vector_search_batch(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                            const float *qvecs, const float *alpha, const float *boost, const int32_t *q_filter,
                            uint32_t cand_size, uint32_t k_out, uint32_t *out_doc, uint32_t *out_seg,
                            float *out_score, float *out_vec_score, uint32_t *out_count, uint64_t *out_total) {
  return guarded([&] {
    vs_staged(ix, nq, n_clauses, clause_field, cand_size, k_out,
              {qvecs, alpha, boost, q_filter, out_doc, out_seg, out_score, out_vec_score, out_count, out_total});
  });
}

int slg_vector_search_batch_device(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field,
                                   const float *d_qvecs, const float *d_alpha, const float *d_boost,
                                   const int32_t *d_q_filter, uint32_t cand_size, uint32_t k_out,
                                   uint32_t *d_out_doc, uint32_t *d_out_seg, float *d_out_score,
                                   float *d_out_vec_score, uint32_t *d_out_count, uint64_t *d_out_total) {
  return guarded([&] {
    vs_device(ix, nq, n_clauses, clause_field, cand_size, k_out,
              {d_qvecs, d_alpha, d_boost, d_q_filter, d_out_doc, d_out_seg, d_out_score, d_out_vec_score,
               d_out_count, d_out_total});
  });
}

}  // extern "C"
